/*
 * include/pygmm_hip.h -- C ABI of lib/pygmm.so (MI355X / gfx950 build).
 *
 * Part 1 is a drop-in for the reference's FFI, /root/reference/src/gmm/src/pygmm.hh:11-43:
 * the same ten symbols, the same signatures and argument meaning, so the reference's ctypes
 * caller (src/gmm/python/pygmm.py:16 `cdll.LoadLibrary('../lib/pygmm.so')`) binds it
 * unchanged.  Differences in behaviour, all deliberate:
 *   - nothing throws across the boundary (reference: `throw "literal"`, gmm.cc:45,59,585);
 *     legacy entry points report through sr_last_error() and return NULL / NaN / no-op;
 *   - `concurrency` is accepted and ignored (the HIP grid replaces the thread pool,
 *     gmm.cc:533-560);
 *   - score_instance works (the reference aborts on assert(buffer != NULL),
 *     pygmm.cc:113-117 -> gmm.cc:185).
 * Part 2 (sr_ prefix) is the contiguous / batched / device-resident interface the hot path
 * actually wants; the Python mirror of the reference surface calls these.
 *
 * Plain C types only; no HIP or C++ types cross this boundary.
 */
#ifndef PYGMM_HIP_H
#define PYGMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GMM GMM; /* opaque; reference: class GMM, src/gmm/src/gmm.hh:130-173 */

/* src/gmm/src/pygmm.hh:12-26 (mirrored by ctypes at src/gmm/python/pygmm.py:18-27) */
struct Parameter {
    int nr_instance;
    int nr_dim;
    int nr_mixture;
    double min_covar;
    double threshold;
    int nr_iteration;
    int init_with_kmeans;
    int concurrency;
    int verbosity;          /* >= 1: the reference's progress lines (gmm.cc:588-590, :641); >= 2 (extension): the phase
                               times of every EM / MAP iteration on stdout */
};

/* ---------------- Part 1: legacy symbols (pygmm.hh:28-41) ---------------- */

/* pygmm.hh:28 / pygmm.cc:50-52.  covariance_type must be 1 (COVTYPE_DIAGONAL, gmm.hh:18-22). */
GMM *new_gmm(int nr_mixture, int covariance_type);
/* pygmm.hh:29 / pygmm.cc:54-56 -> GMM::load, gmm.cc:664-682 (text format, gmm.cc:101-150). */
GMM *load(const char *model_file);
/* pygmm.hh:31 / pygmm.cc:58-61 -> GMM::dump, gmm.cc:655-662 (6 significant digits). */
void dump(GMM *gmm, const char *model_file);
/* pygmm.hh:33 / pygmm.cc:63-83 -> GMMTrainerBaseline::train, gmm.cc:581-653. X_in: nr_instance row pointers. */
void train_model(GMM *gmm, double **X_in, struct Parameter *param);
/* pygmm.hh:34 / pygmm.cc:85-96 -> MAP means-only adaptation, gmmubm.cc:29-81. */
void train_model_from_ubm(GMM *gmm, GMM *ubm, double **X_in, struct Parameter *param);
/* pygmm.hh:36 / pygmm.cc:98-102: sum over frames of the per-frame log-likelihood. */
double score_all(GMM *gmm, double **X_in, int nr_instance, int nr_dim, int concurrency);
/* pygmm.hh:37 / pygmm.cc:104-111: per-frame log-likelihoods into caller-owned prob_out[nr_instance]. */
void score_batch(GMM *gmm, double **X_in, double *prob_out, int nr_instance, int nr_dim, int concurrency);
/* pygmm.hh:38 / pygmm.cc:113-117. */
double score_instance(GMM *gmm, double *x_in, int nr_dim);
/* pygmm.hh:40-41 / pygmm.cc:119-120. */
int get_dim(GMM *gmm);
int get_nr_mixtures(GMM *gmm);

/* ---------------- Part 2: extensions ---------------- */

/* Status: 0 = ok, negative = error (text via sr_last_error(), thread-local). */
const char *sr_last_error(void);

/* Processes.  The reference's drivers fit in the parent and THEN fork a multiprocessing.Pool whose workers score
 * (src/test/test-nperson.py:126-139, src/test/test-gmm.py:120-133); a HIP runtime does not survive fork().  So:
 *   - the runtime is initialised lazily, at the first call that needs the device: a pool forked BEFORE that gives
 *     every worker a runtime of its own;
 *   - a process forked AFTER its parent used the GPU is detected (pthread_atfork + pid).  There the reference's ten
 *     symbols above, sr_score_frames_f32 and sr_train_f32 keep working -- they are served by a helper process
 *     (lib/sr_fork_helper next to lib/pygmm.so, spawned at the first such call, one per forked child; csrc/fork_proxy.cpp)
 *     with the results of the in-process path; every other entry point that needs the device returns its error
 *     status with a message naming the remedy, without touching HIP; host-only entry points (load / dump / new_gmm /
 *     get_* / sr_gmm_* / sr_mfcc_tables ...) work as always; inherited device handles may be freed (a no-op there).
 * sr_gpu_runtime_lost() = 1 in such a process.  Pinned by tests/test_fork.py (CPU) and tests/test_gpu_fork.py. */
int sr_gpu_runtime_lost(void);

/* Device plumbing.  One process may drive several GPUs:
 * every host thread has a current device; stream, workspaces, timers and the entry-point lock exist
 * once per device, so threads on different devices run in parallel and threads sharing a device are
 * serialised.  Handles that own device memory (SRBatch, SRModelSet, SRStream) belong to the device
 * they were created on and refuse calls from a thread that is on another one.
 * sr_set_device: the process default (what threads that never chose get) and the calling thread's;
 * sr_set_thread_device: the calling thread's only. */
int sr_device_count(void);
int sr_set_device(int device);
int sr_set_thread_device(int device);
int sr_get_device(void);
int sr_device_synchronize(void);
int sr_device_name(char *buf, int buflen);
/* NUMA: the node of `device` per sysfs (-1: unknown); sr_bind_thread_near_device pins the CALLING host thread to that node's
 * cores and returns the node (-1: left alone).  The slot threads of sr_multi_* do it themselves. */
int sr_device_numa_node(int device);
int sr_bind_thread_near_device(int device);

/* Model handles beyond the legacy constructors. */
void sr_free_gmm(GMM *gmm);
GMM *sr_gmm_from_arrays(int nr_mixture, int nr_dim, const double *weights, const double *mean,
                        const double *sigma);                       /* sigma = std deviations */
int sr_gmm_get_params(GMM *gmm, double *weights, double *mean, double *sigma);
int sr_gmm_dumps(GMM *gmm, char *buf, long buflen, long *needed);     /* text format into memory */
GMM *sr_gmm_loads(const char *text);

/* Contiguous fp32 scoring of ONE model (frames row-major [n][dim], host memory).
 * flags: SR_CLAMP_COMPAT reproduces the reference's underflow behaviour: its densities and its mixture
 * sum are formed in the linear domain under FTZ arithmetic, so a term w_k p_k(x) below DBL_MIN =
 * exp(-708.396) counts as 0 and an all-zero sum returns ln(1e-15) (gmm.cc:34-38, :237-244; pinned by
 * reference-DSO vectors, tests/golden/make_clamp_golden.py) -- and so does a term any PARTIAL product of
 * which dips below DBL_MIN (gmm.cc:192-195), or one dimension of which reaches the exponent floor of
 * fastexp.cc:104-131, although its full product would be representable.  The frames this can matter
 * for (log-likelihood within a few tens of nats of -708.4: frames ~37 sigma from every mixture) are found
 * by every engine and re-evaluated with the reference's own arithmetic (csrc/gmm_flush.hip; pinned by
 * tests/golden/make_flush_golden.py on the DSO).  Which partial products exist is the compiler's choice under
 * the reference's -ffast-math: option "flush_order" 2 (default) = the DSO as g++ 11 builds it from the
 * reference's flags (even / odd dimension lanes), 1 = the source's order.
 * SR_SCORE_PRECISE keeps to the fp32-grade engines (the split-fp16 ones carry 22 significand bits). */
#define SR_CLAMP_COMPAT 1
#define SR_SCORE_PRECISE 0x200
int sr_score_frames_f32(GMM *gmm, const float *X, long n, int dim, float *ll_out, double *sum_out,
                        int flags);

/* All of `models` on ONE utterance in one fused pass: sums_out[i] = the sum over the frames of model i's log-likelihood -- what
 * the reference's per-speaker loop of score_all calls computes (gmmset.py:95-99).  The packed set of the last model list is
 * kept (keyed by the handles and their parameters' state), so a loop over utterances packs once.  Unlike SRModelSet handles this
 * entry point also works in a process forked after its parent used the GPU (the reference's Pool drivers,
 * test-nperson.py:126-146): there it is ONE conversation with the process's helper instead of one per model. */
int sr_score_models_f32(GMM *const *models, int n_models, const float *X /* [n_frames][dim] */, long n_frames, int dim,
                        double *sums_out /* [n_models] */, int flags /* SR_CLAMP_COMPAT | ... */);

/* Speaker set: S models packed once, resident in HBM (replaces the per-speaker ABI loop of
 * src/testbench/gmmset.py:59-64,95-99). */
typedef struct SRModelSet SRModelSet;
SRModelSet *sr_modelset_create(GMM *const *models, int n_models);
void sr_modelset_free(SRModelSet *set);
int sr_modelset_size(SRModelSet *set);
/* Conditioning of the packed set as the engine dispatcher sees it: out8[0] = amp = max_k sum_d
 * ((mu_kd - centre_d) / sigma_kd)^2 (the cancellation the expanded quadratic form has to survive in
 * fp32), [1] = dead fraction of the 32-mixture tiles, [2] = largest per-dimension sigma ratio,
 * [3] = largest scaled coefficient of the fp16 layouts, [4] = 1 if sigma and weights are shared,
 * [5] = models, [6] = device, [7] = mixtures (of the largest model) that the hybrid form sends to the
 * direct-form vector engine because the expanded form would cancel for them (0: no hybrid form; the other
 * entries then describe the whole set).  A set that is ill conditioned because of a few mixtures only -- collapsed
 * components at the sigma floor -- is scored as two sub-sets whose per-frame values are merged by a log-add-exp. */
int sr_modelset_info(SRModelSet *set, double *out8);
int sr_modelset_dim(SRModelSet *set);

/* Utterance batch resident in HBM: either PCM (int16, concatenated, sample_offsets[U+1]) or
 * features (fp32 [n][dim], frame_offsets[U+1]). */
typedef struct SRBatch SRBatch;
SRBatch *sr_batch_from_pcm(const int16_t *pcm, const int64_t *sample_offsets, int n_utt);
SRBatch *sr_batch_from_pcm_f32(const float *pcm, const int64_t *sample_offsets, int n_utt);
SRBatch *sr_batch_from_features(const float *X, int64_t n_frames, int dim,
                                const int64_t *frame_offsets, int n_utt);
/* Overwrite the samples of a PCM batch in place (same utterance layout, same or fewer samples per
 * utterance is NOT supported: the layout must match exactly) -- the serving loop's H2D, no allocation.
 * Up to 4 MB of samples are copied to a page-locked staging area and the call returns with the transfer in
 * flight on the library's stream (the caller's buffer may be reused at once; whatever is queued next on the
 * stream -- sr_predict_pcm_batch, sr_mfcc_extract_batch -- runs behind it); larger updates return when the
 * samples are on the device. */
int sr_batch_update_pcm(SRBatch *b, const int16_t *pcm, int64_t n_samples);
/* New contents AND a new utterance layout in the same handle: device buffers are reused (they only
 * grow), so a serving loop whose batches change shape allocates nothing in steady state.  Up to 4 MB of samples travel as
 * sr_batch_update_pcm's do -- page-locked copy, transfer left in flight, the caller's buffers free on return -- together with
 * their offsets; the feature stage's and the scoring pass's tables of such a batch are rebuilt the same way (no host wait). */
int sr_batch_reset_pcm(SRBatch *b, const int16_t *pcm, const int64_t *sample_offsets, int n_utt);
/* The same for a feature batch: new frames and a new utterance layout (any dim) in the handle's buffers -- what keeps the
 * reference's per-utterance loop (gmmset.py:62-64, :95-99: one scoring call per utterance) free of allocations.  Up to 4 MB of
 * frames are copied to a page-locked staging area and the call returns with the transfer in flight on the library's stream (X is
 * the caller's again at once; sr_score_batch_set and whatever else is queued next runs behind it); larger refills return when the
 * frames are on the device. */
int sr_batch_reset_features(SRBatch *b, const float *X, int64_t n_frames, int dim,
                            const int64_t *frame_offsets, int n_utt);
void sr_batch_free(SRBatch *b);
int sr_batch_num_utterances(SRBatch *b);
int64_t sr_batch_num_rows(SRBatch *b);           /* samples (PCM) or frames (features) */
int sr_batch_dim(SRBatch *b);                    /* 0 for PCM */
int sr_batch_offsets(SRBatch *b, int64_t *offsets_out /* [U+1] */);
int sr_batch_download(SRBatch *b, float *out);   /* features -> host, [rows][dim] */
int sr_batch_download_pcm16(SRBatch *b, int16_t *out);   /* PCM16 batches -> host, [rows] */

/* Energy-threshold silence removal (csrc/silence.hip), the reference's src/filters/silence.py:11-50 -- what its corpus
 * preparation applies to every recording -- on every utterance of a PCM16 batch; the result is a new PCM16 batch on the same
 * device, fit for sr_mfcc_extract_batch / sr_predict_pcm_batch without a host round trip.  Per utterance of n samples, with
 * L = int(frame_duration * fs) and S = int(frame_shift * fs): A = (sum x^2) / n; from i = 0 while i < n the frame x[i : i + L]
 * (clipped at n, len samples) is silent when (sum frame^2) / len < A * perc -- exact integer sums, the comparison strict and in
 * float64 -- and i += L; otherwise its first min(S, len) samples are appended and i += S.  Bit-identical to the reference for
 * int16 input (the reference's defaults: 0.02, 0.01, 0.15).  An utterance may come out with 0 samples (perc >= 1); the feature
 * stage gives it 0 frames and the fused calls argmax -1.
 * kept_out: [U] kept samples per utterance, or NULL.  NULL + sr_last_error() on refusal: a PCMF32 or FEATURES batch, a batch
 * without utterances, an utterance without samples, L < 1 or S < 1 (the reference loops forever or raises there).
 * sr_set_option("silence_block", B): positions (multiples of gcd(L, S) samples) per block of the walk, 0 = automatic. */
SRBatch *sr_silence_remove_batch(SRBatch *pcm, double fs, double frame_duration, double frame_shift, double perc,
                                 int64_t *kept_out);
/* What such a call decides for a longest utterance of max_samples (csrc/silence_plan.cpp; host only, no GPU needed), for tests.
 * Writes 12 fields (n_out >= 12; values above INT32_MAX saturate) and returns 12, -1 on refusal: L, S, g = gcd(L, S),
 * E = entries of a block's transfer map = min(max(L, S) / g, positions), B = positions per block, blocks of that utterance,
 * variant (0: a lane per (block, entry), several blocks per workgroup; 1: E above the workgroup, lanes loop over the entries),
 * blocks per workgroup, kept frames a block can list, grid of the maps launch for that utterance alone, lanes per position of
 * the energy kernel, positions of that utterance. */
int sr_silence_plan(double fs, double frame_duration, double frame_shift, int64_t max_samples, int32_t *out, int n_out);

/* Short-time feature normalisation (csrc/featnorm.hip) of every utterance of a FEATURES batch, each utterance and each column on
 * its own; the result is a new FEATURES batch of the same layout on the same device.  An utterance of T frames and a window of
 * `window` = W frames (2 .. 1024, even or odd): frame t looks at the N = min(W, T) rows from s0(t) = min(max(t - W / 2, 0), T - N)
 * -- centred in the interior, shifted (not shortened) at both ends.
 *   mode 0, warp (Pelecanos & Sridharan 2001): less = values of the window < x_t, eq = values == x_t (fp32 comparisons, the frame
 *     itself included), the doubled mid-rank r2 = 2 less + eq - 1, out = (float) Q((r2 + 1) / (2 N)) with Q the standard normal
 *     quantile (sr_norm_quantile), taken through the lower half of the distribution: ranks mirrored about the middle give values
 *     that are each other's negatives to the bit, a constant stretch gives exactly 0.  A NaN cell gives NaN and rank -1 and is
 *     counted; a NaN neighbour is neither less nor equal; +-inf rank like any value.
 *   mode 1, cmn: out = (float)(x_t - mean), mean = (sum x) / N in float64, summed in window order.
 *   mode 2, cmvn: out = (float)((x_t - mean) / sqrt(var)), var = (sum (x - mean)^2) / N, the second pass in window order too (the
 *     population variance, no epsilon).  A window whose values all compare equal gives exactly 0 and is counted.  NaN propagates.
 * degenerate_out: [U] counts (warp: NaN cells; cmvn: equal-valued windows; cmn: 0), or NULL.  ranks_out: host memory, [rows][dim]
 * int32 r2 (warp only), or NULL -- for tests.  An utterance's output is the same bits alone, in any batch, under any "norm_tile"
 * and from run to run.  Utterances of 0 rows stay empty.  NULL + sr_last_error() on refusal, before the device is touched: a PCM
 * batch, a mode outside 0 .. 2, a window outside 2 .. 1024, ranks_out with another mode than 0; a process forked after its parent
 * initialised the GPU runtime is refused as well.  Timed under SR_T_CMVN (no timer kind is added).
 * sr_set_option("norm_tile", F): frames per workgroup, a multiple of 64 up to 1024; 0 = automatic (256). */
SRBatch *sr_feature_norm_batch(SRBatch *feats, int mode, int window, int64_t *degenerate_out, int32_t *ranks_out);
/* What such a call decides for columns of width dim and a longest utterance of max_frames under the current "norm_tile"
 * (csrc/featnorm_plan.cpp; no GPU needed when n_cu > 0; n_cu <= 0: the current device's).  Writes 12 fields (n_out >= 12) and
 * returns 12, -1 on refusal: frames per workgroup F, rows a workgroup stages at most, floats between two columns in LDS, columns
 * per pass, passes, LDS bytes, workgroups of that utterance alone, the grid for it, 1 when the warped values of full windows come
 * from a table, that table's length, lanes per workgroup, the largest window built. */
int sr_feature_norm_plan(int mode, int window, int dim, int64_t max_frames, int n_cu, int32_t *out, int n_out);
/* The standard normal quantile in float64: Wichura's AS241 (PPND16), the host instance of the function the kernels evaluate.
 * 0 < p < 1; NaN otherwise. */
double sr_norm_quantile(double p);

/* Score every utterance of a feature batch against every model of the set in one fused pass:
 * sums_out[U][S] = sum_t LL_s(x_t) (double), argmax_out[U] = first maximum (gmmset.py:62-64),
 * frame_ll_out (optional, may be NULL) = [S][n_frames] fp32 per-frame log-likelihoods. */
int sr_score_batch_set(SRModelSet *set, SRBatch *features, double *sums_out, int *argmax_out,
                       float *frame_ll_out, int flags);

/* MFCC extractor (src/feature/MFCC.py:20-41 constants; :49-79 chain; utils.py:24-31 deltas). */
typedef struct SRMfcc SRMfcc;
SRMfcc *sr_mfcc_create(double fs, double win_length_ms, double win_shift_ms, int fft_size,
                       int n_filters, int n_ceps, double pre_emphasis);
/* n_lpc > 0: append LPC-n_lpc columns to every frame (the reference's mix_feature,
 * src/feature/__init__.py:25-30 -> LPC.py:40-57; same framing, no deltas); 0 switches them off. */
int sr_mfcc_set_lpc(SRMfcc *m, int n_lpc);
void sr_mfcc_free(SRMfcc *m);
int sr_mfcc_frame_len(SRMfcc *m);
int sr_mfcc_frame_shift(SRMfcc *m);
int64_t sr_mfcc_num_frames(SRMfcc *m, int64_t n_samples);   /* MFCC.py:57; 0 if too short (:56) */
int sr_mfcc_tables(SRMfcc *m, double *window /*[L]*/, double *melbank /*[n_filters][fft/2+1]*/,
                   double *dct /*[n_ceps][n_filters]*/);    /* host float64 tables, for tests */
/* What a pass of n_frames > 0 frames launches (csrc/mfcc_plan.cpp), for tests: precision 2 / 0 and generic 0 / 1 as the options
 * mfcc_precision and mfcc_generic take them, pcm_kind 0 = int16, 1 = float32; n_cu > 0: that many compute units (host only, no GPU
 * needed), n_cu <= 0: the current device's.  Writes 16 fields (n_out >= 16) and returns 16: kernel (0 fp32 fast, 1 fp32 generic,
 * 2 float64 fast, 3 float64 generic), N1, NZ1, mel preset, waves per workgroup, dynamic LDS bytes, frames per wave, grid,
 * cmvn_delta_kernel's column padding, floats of the padded mel table, its four pass lengths, the largest float index of the power
 * spectrum a padded sweep reads, the number of empty mel bands. */
int sr_mfcc_plan(SRMfcc *m, int precision, int generic, int pcm_kind, int64_t n_frames, int n_cu, int32_t *out, int n_out);
/* PCM batch -> feature batch (CMVN per utterance, then delta order nd in {0,1,2});
 * cmvn=0 skips the normalisation (raw cepstra and their plain differences, for tests). Returns a new device batch. */
SRBatch *sr_mfcc_extract_batch(SRMfcc *m, SRBatch *pcm, int nd, int cmvn);

/* Fused serving step on resident inputs: PCM batch -> MFCC -> CMVN/delta -> scoring -> argmax. */
int sr_predict_pcm_batch(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out,
                         int *argmax_out, int flags);

/* Every GPU of the node from ONE host process (no torch, no MPI, no collective): utterances are dealt
 * to n_slots slots by length, slot i lives on device i % sr_device_count() with its own replica of
 * the models and extractor tables, one host thread per slot runs upload -> MFCC -> CMVN/deltas -> all
 * models -> sums + argmax, and the per-utterance rows are gathered on the host (the reference:
 * Threadpool inside the call, gmm.cc:533-560, and multiprocessing.Pool over utterances,
 * test-gmm.py:128-133).  n_slots = 0 means one slot per visible device; more slots than devices is
 * legal: slots that share a device are one queue on it (the first of them takes their work and the others report 0
 * seconds; sr_set_option("multi_merge_same_device", 0) gives every slot its own thread and share, serialised by the
 * device's lock).  slot_seconds_out (optional, [n_slots]) receives each slot's wall time for the pass. */
typedef struct SRMulti SRMulti;
SRMulti *sr_multi_create(GMM *const *models, int n_models, double fs, double win_length_ms,
                         double win_shift_ms, int fft_size, int n_filters, int n_ceps,
                         double pre_emphasis, int n_slots);
void sr_multi_free(SRMulti *m);
/* Page-lock caller memory (hipHostRegister) -- a serving loop's PCM ring, say -- so that sr_multi_predict_pcm's copy
 * engines read it in place instead of going through a staging buffer; sr_host_unregister before it is freed. */
int sr_host_register(void *p, size_t bytes);
int sr_host_unregister(void *p);
int sr_multi_slots(SRMulti *m);
int sr_multi_slot_device(SRMulti *m, int slot);
int sr_multi_slot_numa_node(SRMulti *m, int slot);      /* where the slot's host thread was pinned in its last pass (-1: nowhere) */
int sr_multi_slot_pieces(SRMulti *m, int slot);         /* pieces the slot cut its utterances into in the last call (0: it took no work) */
int sr_multi_predict_pcm(SRMulti *m, const int16_t *pcm, const int64_t *sample_offsets, int n_utt,
                         int nd, double *sums_out /*[U][S]*/, int *argmax_out /*[U]*/,
                         double *slot_seconds_out, int flags);
/* sr_multi_plan: what such a call decides before it touches a device (csrc/multi_plan.cpp; host only), for tests.  devices:
 * [n_slots] the slots' device indices; merge: the option multi_merge_same_device; schedules: [n_slots] every slot's piece schedule
 * (0 = nearly equal pieces, 1 = growing ones; NULL: 0 for all).  Returns the number A of slots that take work, -1 on bad arguments.
 * active_out [n_slots]: their slot indices; counts_out [n_slots]: utterances of each; utts_out [n_utt]: their utterance lists, one
 * after the other, each ascending; pieces_out [n_slots][17]: per active slot the number of pieces n, then (u0, u1) of 8 pieces --
 * ranges of the slot's list, a contiguous cover of it. */
int sr_multi_plan(const int64_t *sample_offsets, int n_utt, const int *devices, int n_slots, int merge, const int *schedules,
                  int *active_out, int *counts_out, int *utts_out, int *pieces_out);

/* Measured device-to-device copy rate (bytes read + written per second, GB/s) of a `bytes`-sized
 * buffer over `iters` copies on the library's stream: the HBM ceiling bench.py quotes beside the
 * nominal 8 TB/s. */
int sr_hbm_copy_gbps(size_t bytes, int iters, double *gbps_out);

/* Fixed-shape serving session: n_windows windows of window_samples int16 samples per tick.  Two
 * slots of pinned + device buffers and a second HIP stream: the H2D copy of tick i+1 overlaps the
 * kernels of tick i.  submit() returns after queueing (at most two ticks in flight); collect()
 * waits for the oldest tick and hands back sums[n_windows][S], argmax[n_windows] and the
 * device-side time from the start of its H2D to its last kernel. */
typedef struct SRStream SRStream;
#define SR_STREAM_GRAPH 0x100   /* flags: replay each tick's kernels + result copies as one hipGraph */
SRStream *sr_stream_create(SRMfcc *m, SRModelSet *set, int n_windows, int64_t window_samples, int nd,
                           int flags);
int sr_stream_submit(SRStream *s, const int16_t *pcm /* [n_windows][window_samples] */);
int sr_stream_collect(SRStream *s, double *sums_out, int *argmax_out, double *device_ms);
void sr_stream_free(SRStream *s);

/* Long-term spectral divergence of half-overlapped Hann windows -- the measure behind the reference's
 * voice-activity front end (src/filters/ltsd.py:32-64, which calls third-party pyssp.vad.ltsd; the
 * algorithm is restated from its published form, parity unpinned).  winsize = int(0.04644 * fs)
 * (ltsd.py:17,66-69), hop winsize/2, windows per signal = len/(winsize/2) - 1.
 * sr_ltsd_noise_spectrum: mean amplitude spectrum (bins 0..winsize/2) over all windows of `noise`.
 * sr_ltsd_compute: LTSD in dB of every window of every utterance of `pcm` against that spectrum;
 * ltsd_out holds win_offsets_out[U] floats, utterance u's windows at [win_offsets_out[u], win_offsets_out[u+1]). */
int64_t sr_ltsd_num_windows(int64_t n_samples, int winsize);
int sr_ltsd_noise_spectrum(SRBatch *noise, int winsize, float *avg_amp_out /*[winsize/2+1]*/);
int sr_ltsd_compute(SRBatch *pcm, int winsize, int order, const float *noise_amp /*[winsize/2+1]*/,
                    float *ltsd_out, int64_t *win_offsets_out /*[U+1]*/);

/* GPU EM / MAP on contiguous fp32 frames (the engine behind train_model*). Returns the number
 * of iterations run, negative on error. seed < 0 -> time-based. */
int sr_train_f32(GMM *gmm, GMM *ubm_or_null, const float *X, long n, int dim,
                 const struct Parameter *param, long seed);

/* ---- A set of speakers MAP-adapted from ONE UBM in one batched device fit (csrc/map_batch.hip) ----
 * S >= 1 handles (new_gmm; their mixture count is replaced by the UBM's, as train_model_from_ubm does) fitted together on the
 * speakers' frames X ([row_offsets[S]][dim] fp32, speaker s owns rows row_offsets[s] .. row_offsets[s + 1]): every pass is one
 * set of launches for a whole group of speakers, the stop rule (gmm.cc:622-650) is applied per speaker on the device, and the host
 * reads one word -- the speakers still active -- where the rule is taken.  Every fitted speaker's model and iterations_out[s] are
 * the bits and the count sr_train_f32(models[s], ubm, its rows, ...) gives for that speaker alone, for every batch size, order of
 * speakers and scratch bound.  status[s]: 0 fitted in the batch; 1 fitted by the single fit (its shape is outside the float64
 * iteration engine's, or speaker-sized: the whole-fit kernel's); 2 handed over (a live frame near the underflow boundary or a NaN
 * density: refitted alone, the iteration-at-a-time path, as its single fit takes it); -1 failed (the handle keeps its parameters;
 * sr_map_fit_batch_error(s) gives the reason -- a speaker without frames: "X.size() == 0").  A failing speaker fails alone.
 * Returns the number of speakers fitted, or -1 when the call itself is refused (sr_last_error()); every argument is checked before
 * the device is touched: no null pointer, S >= 1, offsets from 0 that do not decrease, a trained UBM of `dim` dimensions, no handle
 * twice.  With param->verbosity >= 1, "reference_side_effects" on or "em_stats_engine" != 0 the whole call runs as single fits.
 * seed < 0: libc's stream advances by 1 + K per fitted speaker, as the loop of single fits advances it.  The batched speakers run
 * in groups whose float64 scratch stays under sr_set_option("map_fit_batch_bytes", bytes) (>= 1; default 1 GiB; a speaker above
 * it is a group of its own); the cut does not show in any result.  Fails in a process forked after GPU initialisation. */
int sr_map_fit_batch(GMM *const *models, int S, GMM *ubm, const float *X, const int64_t *row_offsets, int dim,
                     const struct Parameter *param, long seed, int *iterations_out, int *status);
/* Why speaker s of the calling thread's last sr_map_fit_batch failed ("" when it did not, or s is out of range).  The pointer is
 * valid until that thread's next sr_map_fit_batch. */
const char *sr_map_fit_batch_error(int s);
/* Counters since the library was loaded: sr_map_fit_batch calls that reached the device, the speakers fitted in a batch, by the
 * single fit (routed there) and handed over, and the passes launched (one per set of launches, whatever the number of speakers in
 * it).  Any pointer may be NULL. */
void sr_map_fit_batch_stats(long *calls, long *speakers_batched, long *speakers_single, long *speakers_handed_over, long *passes);
/* The current value of the option "map_fit_batch_bytes". */
long sr_map_fit_batch_bytes(void);
/* What such a call decides (csrc/map_plan.cpp; host only when n_cu > 0, n_cu <= 0: the current device's), for tests.  out [12]:
 * speakers batched, single, failing, groups, rows of the density table, rows of the chunk table, mixture blocks (the grids' y),
 * LDS bytes of a density / a statistics workgroup, the largest group's scratch bytes, rounds of its density launch over the chip,
 * doubles of a speaker's state.  speakers_out [S][6] (may be NULL): route (0 batched, 1 single, -1 failing), group, slot in the
 * group, frames padded to whole density tiles, 64-frame chunks, scratch bytes.  groups_out [group_cap][6] (may be NULL): first
 * speaker, speakers, density tiles (grid x), chunks (grid x), scratch bytes, first row of the density table.  tiles_out /
 * chunks_out [cap][3] (may be NULL): speaker, its first row in the batch, local tile.  Returns 12, or -1 with the reason. */
int sr_map_fit_plan(int K, int D, const int64_t *lengths, int S, const struct Parameter *param, int64_t scratch_bytes, int n_cu,
                    int64_t *speakers_out, int64_t *groups_out, int64_t group_cap, int64_t *tiles_out, int64_t tile_cap,
                    int64_t *chunks_out, int64_t chunk_cap, int64_t *out, int n_out);

/* Kernel timing by HIP events on the library's own stream.  (The batched passes of sr_map_fit_batch count under SR_T_ESTEP.) */
#define SR_T_SCORE 0
#define SR_T_MFCC 1
#define SR_T_CMVN 2
#define SR_T_FINALIZE 3
#define SR_T_ESTEP 4
#define SR_T_SCORE_REF 5   /* reference-offset pre-pass of the split-fp16 shared-sigma engine */
#define SR_T_TOPC_SELECT 6   /* the four stages of sr_score_batch_set_topc (csrc/gmm_topc.hip) */
#define SR_T_TOPC_ROUTE 7
#define SR_T_TOPC_EVAL 8
#define SR_T_TOPC_COMBINE 9
#define SR_T_BW_LSE 10       /* the three passes of sr_bw_stats_batch (csrc/bw_stats.hip): per-frame log-sum-exp, */
#define SR_T_BW_STATS 11     /* the statistics on the fp64 matrix cores, */
#define SR_T_BW_REDUCE 12    /* the sum of an utterance's slabs */
#define SR_T_JFA_GRAM 13     /* the stages of sr_jfa_factors / _update / _train (csrc/jfa.hip): W ./ E and the gram matrices P, */
#define SR_T_JFA_GEMM_L 14   /* the float64 matrix-core GEMM's four products: L = I + N P, */
#define SR_T_JFA_GEMM_B 15   /* b = Fc (W ./ E)^T, */
#define SR_T_JFA_GEMM_A 16   /* A += N^T Q, */
#define SR_T_JFA_GEMM_C 17   /* C += Y^T Fc, */
#define SR_T_JFA_FACTOR 18   /* the batched factorisation of the groups' blocks, */
#define SR_T_JFA_UPDATE 19   /* the factorisation and solve of the mixtures' blocks */
#define SR_T_COUNT 20
int sr_profile_enable(int on);
int sr_profile_reset(void);
int sr_profile_get(int kind, double *total_ms, long *launches);

/* Options (process-wide; value 0 = automatic unless stated).  The complete table -- key, values, default, the test that pins it --
 * is DESIGN.md section 8.  The ones a caller may want:
 *   "mfcc_precision" 2 (default: float64 spectrum, ln and DCT for every frame, the reference's arithmetic) | 0 (fp32 throughout,
 *                    ~1.5x faster feature stage; cepstra up to 2e-2 off on voices whose mel bands lie > 60 dB apart),
 *   "score_engine"   1 vector ALU | 3 split-bf16 | 4 split-bf16 shared-sigma | 5 split-fp16 | 6 split-fp16 shared-sigma,
 *   "flush_order"    2 | 1 (see SR_CLAMP_COMPAT),
 *   "reference_side_effects" 1: train_model / train_model_from_ubm print the parameter block (pygmm.cc:31-41) and the trainer
 *                    writes ./gmm-training-intermediate-dump.model after every second iteration (gmm.cc:622-630), as the reference
 *                    does unconditionally; 0 (default): neither,
 *   "multi_numa_bind" 0: sr_multi slot threads leave their CPU affinity alone (default 1: bound to the cores of their GPU's NUMA
 *                    node, intersected with the mask the thread already has),
 *   "multi_merge_same_device" 0: slots that share a device get a host thread each (default 1: one queue per device).
 *   "full_fit_batch_bytes" the workspace bound, in bytes (>= 1; default 1 GiB), of a group of speakers in sr_fullgmm_fit_batch.
 *   "map_fit_batch_bytes" the bound, in bytes (>= 1; default 1 GiB), of the float64 scratch of a group of speakers in sr_map_fit_batch.
 *                    Results do not depend on it, bit for bit.
 *   "silence_block"  positions per block of sr_silence_remove_batch's walk (1 .. 2^30; 0 = automatic: max(256, 4 E, positions of the longest utterance / 2048)).
 *   "norm_tile"      frames per workgroup of sr_feature_norm_batch (a multiple of 64 up to 1024; 0 = automatic: 256).  Results do not
 *                    depend on it, bit for bit.
 *   "topc_scratch_mib" the scratch bound of sr_score_batch_set_topc, in MiB (>= 1; default 1024): the pass runs in chunks of frames that fit.
 *   "bw_scratch_mib" the bound, in MiB (1 .. 2^20; default 1024), of the float64 slabs sr_bw_stats_batch keeps at a time: the range
 *                    table runs in groups that fit.  Results do not depend on it, bit for bit.
 *   "bw_range_frames" frames per range of sr_bw_stats_batch (1 .. 2^30; 0 = automatic: max(1024, the utterance's length / 256 rounded
 *                    up to whole tiles of 128)).  Results depend on it in their last bits only.
 *   "jfa_scratch_mib" the bound, in MiB (1 .. 2^20; default 1024), of the R x R float64 blocks sr_jfa_factors / _train keep at a time:
 *                    the groups run in chunks that fit.  Results do not depend on it, bit for bit.
 *   "norm_scratch_mib" the bound, in MiB (1 .. 2^20; default 1024), of the scratch of sr_score_norm's as2 mode (the selections, the shifted
 *                    copies and the four products): the test segments run in chunks that fit.  Results do not depend on it, bit for bit.
 *   "plda_scratch_mib" the bound, in MiB (1 .. 2^20; default 1024), of what sr_plda_score keeps per test segment (its centred row, its row
 *                    of X P_c and its two quadratic forms): the segments run in chunks that fit.  Results do not depend on it, bit for bit.
 *   "calib_scratch_mib" the bound, in MiB (1 .. 2^20; default 8192), of what a calibration call (sr_calib_train / _eval / _apply / _counts)
 *                    keeps resident on the device: the scores, the labels and the blocks' partial sums.  A call above it is refused.
 *                    Results do not depend on it, bit for bit.
 *   "jfa_lds_rows"   largest R whose blocks the JFA factorisation copies into LDS (1 .. 112; 0 = automatic: 112); above it the
 *                    block is factored in place in global memory with panels in LDS.  1 forces that path at any R > 1.
 * The rest select kernel variants for A/B runs and tests. */
int sr_set_option(const char *key, long value);
/* Counters of the partial-product path since the library was loaded: resolve calls, (frame tile, model) pairs
 * noted by the engines, frames re-evaluated.  Any pointer may be NULL. */
void sr_flush_stats(long *calls, long *pairs, long *frames);
/* Counters of the k-means initialiser's nearest-centre search since the library was loaded: full searches taken the fast
 * way (one fused multiply-add per point, centre and dimension; sr_set_option("kmeans_assign_engine", 1) turns it off) and
 * the points those left to the exact pass (near-ties; same results bit for bit).  Either pointer may be NULL. */
void sr_kmeans_fast_stats(long *passes, long *rechecked);
/* Diagnostic for the roofline record: runs v_mfma_f32_32x32x16_f16 chains, nothing else, on every SIMD of the current
 * device for about ms_target milliseconds and reports the executed TFLOP/s and the shader clock they ran at -- the matrix
 * throughput this device sustains under its power cap (MI355X: ~1.6 PFLOP/s at ~1.55 GHz against the 2.5 PFLOP/s that
 * 2.4 GHz would give).  Either pointer may be NULL.  0 on success. */
int sr_mfma_peak_probe(double ms_target, double *tflops, double *mhz);
/* The same chains fed the way the scoring kernels feed them: a fresh A fragment read from LDS for every MFMA (8 KiB parameter
 * images, random finite fp16 bit patterns), 8 random B fragments resident in registers, chains of 8 links -- the ceiling of a
 * kernel of that shape under the power cap (the probe above holds both operands in registers for the whole launch, a load no
 * real kernel presents).  Either pointer may be NULL.  0 on success. */
int sr_mfma_streamed_probe(double ms_target, double *tflops, double *mhz);
/* Name of the scoring kernel variant the last scoring call launched (for bench / logs). */
const char *sr_last_score_kernel(void);
/* Which statistics kernel the last EM / MAP iteration of this process ran: 0 none yet, 1 vector ALU, 2 fp64 matrix cores,
 * 3 fp64 matrix cores with the responsibilities on the 16-bit matrix cores (round 4; csrc/em.hip), 4 the whole fit in one launch
 * (speaker-sized models: <= 32 mixtures x <= 40 dims, <= 8192 frames; csrc/em_small.hip), 5 float64 iterations on the device (short
 * data, <= 8192 frames x <= 64 dims, a model of any size: MAP enrolment from a large UBM; csrc/em_f64.hip).  Tests and benches. */
int sr_last_em_stats_engine(void);
/* The first `count` values of the random stream train_model / load draw from when no seed is given: glibc's rand()
 * from its default seed, restated inside the library (the reference draws its initialisation from libc rand():
 * src/gmm/src/random.hh:22-25, gmm.hh:44, kmeansII.cc:94,133; csrc/ref_rand.cpp).  For checks. */
int sr_reference_rand_sample(int *out, int count);

/* ---- Full-covariance GMMs (csrc/gmm_full.hip): scikit-learn's GaussianMixture(covariance_type='full') ----
 * Layout as sklearn's, so parameters convert 1:1: weights[K], means[K][D], precisions_cholesky[K][D][D] (upper triangular P_k,
 * precision = P_k P_k^T), float64, row-major.  1 <= D <= 64, any K >= 1.  lp_k(x) = ln w_k + sum_i ln P_k[i][i] - D/2 ln 2 pi
 * - 1/2 |P_k^T (x - mu_k)|^2; a frame's log-likelihood is the exact log-sum-exp over k (no clamp).  Every call returns a status
 * (0 ok, -1 error: sr_last_error()) or a handle (NULL on error).  In a process forked after GPU initialisation the compute calls
 * fail (no helper-process proxy for these). */
typedef struct SRFullGMM SRFullGMM;
typedef struct SRFullSet SRFullSet;
struct SRFullFitParams {
    double tol;             /* stop when |lower_bound - previous| < tol */
    double reg_covar;       /* added to every covariance's diagonal */
    int max_iter;           /* >= 1 */
    int init_given;         /* 1: the handle's parameters are the initialisation (weights_init / means_init / precisions_init);
                               0: one-hot responsibilities from the library's seeded k-means (kmeans_init.hip) + one M-step */
    long long seed;         /* the k-means stream's seed (>= 0) */
};
struct SRFullFitStats {
    int n_iter;
    int converged;
    double lower_bound;     /* mean log-likelihood of the last E-step */
};
/* A model of K mixtures in D dims; weights / means / prec_chol may all be NULL (no parameters yet: fit it with init_given 0). */
SRFullGMM *sr_fullgmm_create(int K, int D, const double *weights, const double *means, const double *prec_chol);
/* EM in float64 on the device, as GaussianMixture.fit with n_init = 1.  X: [n][D] float64.  A component whose covariance's
 * Cholesky meets a pivot <= 0 fails the fit with scikit-learn's message ("Fitting the mixture model failed because some
 * components have ill-defined empirical covariance ..."); the handle keeps its previous parameters then.  The fit runs as a group
 * of one in sr_fullgmm_fit_batch's driver; it moves none of sr_full_fit_batch_stats' counters, and "full_fit_batch_bytes" does
 * not bear on it. */
int sr_fullgmm_fit(SRFullGMM *g, const double *X, int64_t n, int D, const struct SRFullFitParams *params, struct SRFullFitStats *out);
/* S >= 1 handles of one K and D fitted together: every EM iteration is one set of launches for the whole batch, the stop rule
 * is applied per speaker on the device, and the host reads one small record per speaker and iteration.  X: the speakers' rows
 * one after the other; row_offsets [S + 1] (speaker s owns rows row_offsets[s] .. row_offsets[s + 1]); params / out / status: [S].
 * status[s]: 0 fitted, -1 failed (the handle keeps its previous parameters; sr_fullgmm_fit_batch_error(s) gives the reason, for a
 * pivot <= 0 scikit-learn's "ill-defined empirical covariance" text).  Returns 0 when the call itself ran (even if speakers
 * failed), -1 on a bad argument -- every argument is checked before the device is touched: S >= 1, offsets from 0 that do not
 * decrease, one K and D, no handle twice, and per speaker what sr_fullgmm_fit checks -- or a device error (sr_last_error()).
 * Every fitted speaker's parameters, n_iter, converged and lower_bound are the bits sr_fullgmm_fit gives for that speaker alone,
 * whatever the batch around it.  Large batches are cut into groups of speakers whose workspace stays under
 * sr_set_option("full_fit_batch_bytes", bytes) (default 1 GiB; a single speaker above it is a group of its own); the cut does
 * not show in any result. */
int sr_fullgmm_fit_batch(SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D,
                         const struct SRFullFitParams *params, struct SRFullFitStats *out, int *status);
/* Why speaker s of the calling thread's last sr_fullgmm_fit_batch failed ("" when it did not, or s is out of range).  The pointer
 * is valid until that thread's next sr_fullgmm_fit_batch. */
const char *sr_fullgmm_fit_batch_error(int s);
/* Counters since the library was loaded: sr_fullgmm_fit_batch calls that reached the device, the speakers they carried, and the
 * batch iterations launched (one per set of E- and M-step launches, whatever the number of speakers in it).  Any pointer may be NULL. */
void sr_full_fit_batch_stats(long *calls, long *speakers, long *iterations);
/* The current value of the option "full_fit_batch_bytes". */
long sr_full_fit_batch_bytes(void);
/* What a fit of S speakers of `lengths` frames decides before it touches the device (csrc/full_plan.cpp; no device is touched),
 * for tests.  init_given / max_iter: [S], or NULL (the k-means start / 100).  bound_bytes: 0 means the current
 * "full_fit_batch_bytes".  out [7]: groups, the lengths of the three work lists (density blocks of 32 frames, 256-frame blocks,
 * covariance chunks) over all groups, the LDS bytes of the density kernel, the largest group's workspace bytes, the workspace bytes
 * of a lone speaker of lengths[0] frames.  speakers_out [S][8] (may be NULL): frames, first row in its group, covariance chunks,
 * frames per chunk, offset of its slice of `partial` (doubles), its bytes alone, group, slot.  groups_out [group_cap][28] (may be
 * NULL): first speaker, speakers, rows, where its ranges of the three lists start, max_iter, any k-means start, any given start,
 * bytes, then the element counts of X, w, logw, mu, prec, logdet, cov, lp, lpn, nk, partial, head, the speaker table, the records,
 * the three lists and the labels.  Returns 7, or -1 with the reason. */
int sr_full_fit_plan(int K, int D, const int64_t *lengths, const int *init_given, const int *max_iter, int S, int64_t bound_bytes,
                     int64_t *speakers_out, int64_t *groups_out, int64_t group_cap, int64_t *out, int n_out);
/* K and D of a handle; 1 when it has parameters, 0 when not, -1 on error.  Either pointer may be NULL. */
int sr_fullgmm_info(SRFullGMM *g, int *K, int *D);
/* Copies the parameters out; any pointer may be NULL.  covariances: the last M-step's (zeros for a model built from arrays). */
int sr_fullgmm_get(SRFullGMM *g, double *weights, double *means, double *covariances, double *prec_chol);
void sr_fullgmm_free(SRFullGMM *g);
/* S >= 1 trained models of one dimension packed and uploaded once to the calling thread's device. */
SRFullSet *sr_fullset_create(SRFullGMM *const *models, int S);
/* Every utterance of a feature batch (dim == the set's D) against every model in one pass: sums_out [U][S] float64 per-utterance
 * totals added in a fixed order (the bits depend neither on the batch's other utterances nor on the position), argmax_out [U]
 * (first maximum wins), frame_ll_out [S][n_rows] fp32 or NULL.  sums_out / argmax_out may be NULL. */
int sr_fullset_score_batch(SRFullSet *set, SRBatch *batch, double *sums_out, int *argmax_out, float *frame_ll_out);
void sr_fullset_free(SRFullSet *set);
/* The fused decision on resident PCM: MFCC (+ the extractor's LPC columns, sr_mfcc_set_lpc, nd must then be 0; or + nd orders of
 * deltas) -> scoring -> per-utterance sums and argmax on the device (fullcov_finalize_kernel) -> one copy back.  The extractor's
 * output width must equal the set's D.  sums_out [U][S]: the bits of sr_fullset_score_batch on the same features.
 * argmax_out [U]: the first maximum of sums / frames (float64, as skgmm.GMMSet.predict), -1 for an utterance without frames
 * (sums 0) -- unlike sr_fullset_score_batch's, which compares the plain sums and gives 0 there.  Either pointer may be NULL. */
int sr_fullset_predict_pcm_batch(SRMfcc *m, SRFullSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out);
/* sr_stream_create for a full-covariance set: the same sr_stream_submit / _collect / _free, results as
 * sr_fullset_predict_pcm_batch's.  flags: 0 or SR_STREAM_GRAPH (any other bit fails). */
SRStream *sr_stream_create_full(SRMfcc *m, SRFullSet *set, int n_windows, int64_t window_samples, int nd, int flags);
/* sr_multi_create for full-covariance models: every slot packs its own SRFullSet replica; n_lpc is 0 or an instantiated LPC order
 * (10, 12, 15, 16, 20: mix_feature's columns, nd 0 then).  sr_multi_predict_pcm's results are sr_fullset_predict_pcm_batch's, bit
 * for bit, for any slot count and any cut into pieces (its flags are ignored); the other sr_multi_* calls work as for diagonal sets. */
SRMulti *sr_multi_create_full(SRFullGMM *const *models, int n_models, double fs, double win_length_ms, double win_shift_ms, int fft,
                              int n_filters, int n_ceps, double pre_emph, int n_lpc, int n_slots);

/* A serving session with the voice-activity front end of the reference's conversation loop (ModelInterface.filter, then predict,
 * per window) on the device: per tick and window, LTSD of the window as an utterance of its own (sr_ltsd_compute's values), the
 * double-threshold rule (a voiced run: a maximal run of analysis windows above lambda0 that holds one above lambda1; the float32
 * LTSD value is compared with the float64 threshold), the voiced half-hops moved together, and -- when more than a third of the
 * window is voiced and the voiced samples yield a frame -- the decision the fused call gives for the voiced samples as one
 * utterance: sr_fullset_predict_pcm_batch's bits for a full-covariance set; for a diagonal set the sum of the per-frame values in
 * a fixed order and its first maximum.  A window that is not scored has sums 0 and argmax -1.  Exactly one of `set` and `fullset`
 * is given; nd must be 0; flags: SR_STREAM_GRAPH, and SR_CLAMP_COMPAT for a diagonal set; ltsd_window = int(0.04644 * fs);
 * noise_amp [ltsd_window / 2 + 1] as sr_ltsd_noise_spectrum gives it.  Submit with sr_stream_submit; sr_stream_collect_vad is
 * sr_stream_collect plus voiced_out [n_windows], each window's voiced samples (NULL: not wanted; non-NULL on a session without
 * the front end fails). */
SRStream *sr_stream_create_vad(SRMfcc *m, SRModelSet *set, SRFullSet *fullset, int n_windows, int64_t window_samples, int nd, int flags,
                               int ltsd_window, int order, const float *noise_amp, double lambda0, double lambda1);
int sr_stream_collect_vad(SRStream *s, double *sums_out, int *argmax_out, int *voiced_out, double *device_ms);

/* ---- Open-set decision against a background model (csrc/open_set.hip): the reference's GMMSet.predict_one_with_rejection
 * (src/testbench/gmmset.py:69-81) taken on the device.  The set carries the UBM as one of its columns, `bg` (GMMSet packs it
 * as column 0).  For an utterance of n frames, in float64 and in the reference's order: q[s] = sums[s] / n for every s != bg;
 * best = the first maximum of q (the quotients are compared, the lowest index wins among equals); margin = q[best] - sums[bg] / n;
 * label = best unless margin < threshold, then -1 (the reference's None).  An utterance without frames, or a set without a column
 * besides bg: label -1, margin NaN.  NaN sums go as the reference's max() takes them: a NaN in the first column besides bg is
 * never replaced and is accepted with margin NaN, a NaN elsewhere never wins.  The kernel runs on FINAL sums: behind the
 * pass's finalize and, for utterances with frames in the partial-product band (SR_CLAMP_COMPAT), again behind their patch.
 * Every call checks its arguments before it touches the device: bg inside [0, S), a threshold that is not a NaN, label_out and
 * margin_out both given (sums_out may be NULL).  Diagonal sets only: a full-covariance set has no UBM (the reference's skgmm.GMMSet
 * has no rejection).  In a process forked after GPU initialisation the calls fail.
 * sr_open_set_decide: the rule on sums in host memory ([U][S], n_frames [U] >= 0) -- upload, kernel, one copy back: for callers
 * that hold sums of several passes, and the direct test of the kernel.
 * sr_score_batch_set_open / sr_predict_pcm_batch_open: the passes of sr_score_batch_set / sr_predict_pcm_batch with the decision
 * kernel behind them; labels and margins come back with the sums, in the same single host wait (results always travel by copy).
 * sr_stream_set_open: before the first sr_stream_submit of a diagonal session (plain, SR_STREAM_GRAPH or voice-activity); from then
 * on every tick enqueues the decision behind its finalize -- a captured tick contains it; a voice-activity session takes the frame
 * counts from its device-side table, and a window it does not score gets -1 / NaN.  Rule and threshold are fixed for the session's
 * life: the call fails once a tick was submitted (a new threshold is a new session), so no captured tick ever goes stale.
 * sr_stream_collect_open: sr_stream_collect_vad with label_out / margin_out [n_windows] in place of the argmax (voiced_out: NULL,
 * or [n_windows] on a voice-activity session); sr_stream_collect / _vad keep working on such a session and return the closed-set
 * argmax.
 * sr_multi_predict_pcm_open: sr_multi_predict_pcm's partition and pieces; every slot decides its utterances on its own device. */
int sr_open_set_decide(const double *sums /* [U][S] */, int U, int S, int bg, const int64_t *n_frames /* [U] */, double threshold,
                       int *label_out /* [U] */, double *margin_out /* [U] */);
int sr_score_batch_set_open(SRModelSet *set, SRBatch *features, int bg, double threshold, double *sums_out, int *label_out,
                            double *margin_out, int flags);
int sr_predict_pcm_batch_open(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int bg, double threshold, double *sums_out,
                              int *label_out, double *margin_out, int flags);
int sr_stream_set_open(SRStream *s, int bg, double threshold);
int sr_stream_collect_open(SRStream *s, double *sums_out, int *label_out, double *margin_out, int *voiced_out, double *device_ms);
int sr_multi_predict_pcm_open(SRMulti *m, const int16_t *pcm, const int64_t *sample_offsets, int n_utt, int nd, int bg,
                              double threshold, double *sums_out, int *label_out, double *margin_out, double *slot_seconds_out,
                              int flags);

/* ---- Top-C Gaussian selection (csrc/gmm_topc.hip; Reynolds, Quatieri & Dunn 2000): fast, APPROXIMATE scoring of a set whose
 * models share sigma and weights -- speakers MAP-adapted from one UBM, means only (gmmubm.cc:40-81) -- with the UBM as column
 * `bg`.  Opt-in: no other entry point takes this path.  Per frame x, with 1 <= top_c <= K:
 *   t_k = ln w_k - sum_d ln(sqrt(2 pi) sigma_kd) - sum_d (x_d - mu^bg_kd)^2 / (2 sigma_kd^2), k = 0 .. K - 1;
 *   top(x) = the top_c indices with the largest t_k, in descending order, equal values to the lower index first;
 *   LL_bg(x) = logsumexp over all K of t_k (the background column stays exact);
 *   LL_s(x) = logsumexp over k in top(x) of the same expression with model s's means, for every s != bg.
 * SR_CLAMP_COMPAT: a per-frame value below ln DBL_MIN = -708.396 becomes ln(1e-15) -- the plain threshold only; the
 * partial-product re-evaluation of csrc/gmm_flush.hip belongs to the exact path and does not apply here.
 * sums_out [U][S] = the per-utterance sums in float64 (fixed order: bit-identical from run to run); argmax_out [U] = the first
 * maximum over all columns as sr_score_batch_set returns it, -1 for an utterance without frames; topc_out [n_frames][top_c]
 * (or NULL) = top(x) of every frame; frame_ll_out [S][n_frames] (or NULL).  The sums feed sr_open_set_decide as they are.
 * A frame with a non-finite feature gives NaN sums for its utterance; its selection is still top_c distinct indices in range.
 * top_c == K reproduces sr_score_batch_set within the parity gate (1e-4 max(1, |LL|) per frame).
 * Refused, before the device is touched, with a message that names the remedy: a set that does not share sigma and weights, bg
 * outside [0, S), top_c outside [1, K], a PCM batch given to the feature entry point, rows wider than 64 dimensions, top_c > 8
 * with K > 8192.  fp32 direct form on the vector engine's packed parameters; the per-set tables are packed on first use.
 * The pass runs in chunks of frames whose scratch (4 top_c S bytes per frame and a little more) stays under
 * sr_set_option("topc_scratch_mib", n) (default 1024); the cut shows in the sums' last bits only.
 * sr_predict_pcm_batch_topc: sr_mfcc_extract_batch (CMVN, nd orders of deltas), then the call above; the features stay on the device.
 * sr_topc_plan: what such a call decides (csrc/topc_plan.cpp; host only when n_cu > 0, n_cu <= 0: the current device's), for tests.
 * Writes 16 fields (n_out >= 16; values above INT32_MAX saturate) and returns 16, -1 on refusal: padded row width, register slots
 * of the running selection (0: the rank kernel), scratch bytes per frame, frames per chunk, chunks, entries per evaluate run, entries
 * staged at a time, waves per evaluate workgroup, evaluate grid x (an upper bound of a full chunk's runs) and y, select grid, route
 * grid, lanes of a combine workgroup, frames per combine tile, LDS bytes of the rank kernel, 0. */
int sr_score_batch_set_topc(SRModelSet *set, SRBatch *features, int bg, int top_c, double *sums_out /*[U][S]*/, int *argmax_out /*[U]*/,
                            int *topc_out /*[n_frames][top_c] or NULL*/, float *frame_ll_out /*[S][n_frames] or NULL*/, int flags);
int sr_predict_pcm_batch_topc(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int bg, int top_c, double *sums_out, int *argmax_out,
                              int flags);
int sr_topc_plan(int K, int D, int S, int top_c, int64_t n_frames, int64_t scratch_bytes, int n_cu, int32_t *out, int n_out);

/* ---- Batched Baum-Welch statistics (csrc/bw_stats.hip): the zero- and first-order statistics of every utterance of a feature
 * batch against ONE diagonal model of a set -- the UBM --, what the reference's JFA leg computes one session at a time in MATLAB
 * (src/jfa/collect_suf_stats.m, sc_compute_suf_stats.m) and what supervectors, factor analysis and i-vectors start from.
 * With gamma_k(t) = w_k N(x_t; mu_k, sigma_k^2) / sum_j w_j N(x_t; mu_j, sigma_j^2) for the frames t of utterance u:
 *   N [U][K]     N[u][k]         = sum_t gamma_k(t)
 *   F [U][K * D] F[u][k * D + d] = sum_t gamma_k(t) x_t[d]       (mixture-major: the reference's supervector order)
 *   ll [U] (or NULL)             = sum_t ln sum_j w_j N(x_t; ...)
 *   dropped [U] (or NULL)        = the frames of u that contributed nothing.
 * A frame contributes iff its log-sum-exp is finite: a row holding a NaN or an infinity, or values so large that every density
 * is -inf, adds nothing to N, F and ll and is counted in dropped.  The posteriors are formed in the log domain, so a frame far
 * from every mixture contributes normally -- where the reference's linear-domain quotient is 0 / 0 = NaN.
 * fp32 densities in the vector engine's 2-FMA form, float64 sums on the fp64 matrix cores in a fixed order: an utterance's N,
 * F and ll are the same bits alone, inside any batch and under any "bw_scratch_mib"; "bw_range_frames" (the cut of an utterance
 * into ranges that are summed apart) shows in the last bits only.  An utterance without frames gives zeros.
 * Refused, before the device is touched, with a message that names the remedy: a PCM batch, `model` outside [0, S), rows wider
 * than 40 dimensions, a feature dimension that is not the model's, a scratch bound below one range's slab.  Refused in a
 * process forked after the GPU runtime was initialised.
 * sr_bw_plan: what such a call decides (csrc/bw_plan.cpp; host only when n_cu > 0, n_cu <= 0: the current device's), for tests:
 * the refusals above from (S, model, K, D, batch_is_features, feat_dim), then for utterances of lengths [n_utt] the range table
 * -- up to range_cap triples {utterance, first row of the batch, rows} into ranges_out (or NULL) -- and 12 fields (n_out >= 12):
 * padded row width, blocks of 16 statistic columns, blocks of 64 mixtures, bytes of one range's slab, ranges, ranges per group,
 * groups, grid of the log-sum-exp pass, LDS bytes of a statistics workgroup, reduce workgroups per (utterance, group), rounds
 * of the largest statistics launch over the chip, the automatic range length of a short utterance.  Returns 12, -1 on refusal. */
int sr_bw_stats_batch(SRModelSet *set, int model, SRBatch *feats, double *N /*[U][K]*/, double *F /*[U][K*D]*/,
                      double *ll /*[U] or NULL*/, int64_t *dropped /*[U] or NULL*/);
int sr_bw_plan(int S, int model, int K, int D, int batch_is_features, int feat_dim, const int64_t *lengths, int64_t n_utt,
               int64_t range_frames, int64_t scratch_bytes, int n_cu, int64_t *ranges_out /*[range_cap][3] or NULL*/, int64_t range_cap,
               int64_t *out, int n_out);

/* ---- JFA factor estimation (csrc/jfa.hip): the reference's estimate_y_and_v.m / estimate_x_and_u.m (src/jfa/; MATLAB there, one
 * speaker at a time), which are one computation on different groups of rows -- what the statistics of sr_bw_stats_batch are for.
 * A group g is a speaker (eigenvoices, or the stacked [v; u] of enrolment), or a session (eigenchannels; i-vectors with W = T).
 * With occupancies N [G][K], CENTRED group-summed first-order statistics Fc [G][K * D] (the caller subtracts what the model
 * already explains), variances E [K * D], a loading matrix W [R][K * D] (W_c = the D columns of mixture c), all float64:
 *   P_c = W_c diag(1 / E_c) W_c^T          L_g = I + sum_c N[g][c] P_c          b_g = W (Fc_g ./ E)
 *   y [G][R]      y_g = L_g^-1 b_g         Q_g = L_g^-1 + y_g y_g^T
 *   A [K][R][R]   A_c = sum_g N[g][c] Q_g  C [R][K * D] = sum_g y_g Fc_g^T      update: W_c <- A_c^-1 C_c
 * sr_jfa_open copies N, Fc and E to the device once: they do not change over the iterations of a training run.
 * sr_jfa_factors: y, with A and C (both or neither) the accumulators; bad_groups (or NULL): groups whose L did not factor.
 * sr_jfa_update: the update alone, on accumulators in host memory (sums of several sr_jfa_factors calls); W in: old, out: new.
 * sr_jfa_train: n_iter rounds of factors -> accumulators -> update with W on the device throughout; W and, if asked, the y of the
 * last round (estimated with the W that round started from, as the reference returns it) come back once.  The same bits as n_iter
 * chained sr_jfa_factors + sr_jfa_update calls.  skipped (or NULL): mixtures the last round's update left alone.
 * Stages: the gram matrices P; one float64 GEMM kernel on v_mfma_f64_16x16x4_f64 for L, b, A and C (ragged edges in every
 * dimension); one workgroup per R x R block for Cholesky, two triangular solves, the explicit inverse and Q written over L.  The
 * blocks of a chunk of groups live under "jfa_scratch_mib"; chunks are multiples of the GEMM's reduction step (16) and A and C are
 * summed in group order across them: NO result depends on the bound, bit for bit; a group's y is the same bits alone and inside
 * any batch; two runs are identical.  R up to 512; blocks of up to "jfa_lds_rows" rows are factored in LDS, larger ones in place.
 * Degenerate inputs: a group whose N is all zero has L = I, y = b (0 exactly for centred statistics of no frames) and adds nothing
 * to A; a group whose L does not factor (a pivot <= 0 or not finite: impossible with N >= 0, E > 0 short of overflow) gets y = 0,
 * adds nothing to A and C and is counted -- nothing non-finite is spread; a mixture whose A_c does not factor (A_c = 0 when no
 * group occupies c: the reference's inv() returns Inf there) keeps its old W_c and is counted in skipped.
 * Refused, before the device is touched, with a message that names the remedy: G, K, D or R < 1, R above 512, a non-finite value
 * in N, Fc, E, W (or in A, C given to sr_jfa_update), a negative N, E <= 0, a scratch bound below one chunk of 16 groups (or of
 * all G, if fewer).  Refused in a process forked after the GPU runtime was initialised.
 * sr_jfa_plan: what such a call decides (csrc/jfa_plan.cpp; host only when n_cu > 0, n_cu <= 0: the current device's), for tests.
 * Writes 32 fields (n_out >= 32) and returns 32, -1 on refusal: groups per chunk, chunks, bytes of N, Fc, E (with 1 / E), P, A, C,
 * W (with W ./ E), y (with b), bytes of a chunk's blocks, factorisation path (0 LDS, 1 global memory), largest R of the LDS path,
 * gram grid x y, the grids x y of the L, b, A and C GEMM launches of a full chunk, LDS bytes of the gram, GEMM, factor and update
 * kernels, rounds of a full chunk's factorisation over the chip, the reduction step, the built limits of R and of the LDS path, 0. */
typedef struct SRJfa SRJfa;
SRJfa *sr_jfa_open(int64_t G, int K, int D, const double *N /*[G][K]*/, const double *Fc /*[G][K*D]*/, const double *E /*[K*D]*/);
int sr_jfa_factors(SRJfa *h, const double *W /*[R][K*D]*/, int R, double *y /*[G][R]*/, double *A /*[K][R][R] or NULL*/,
                   double *C /*[R][K*D] or NULL*/, int64_t *bad_groups /*or NULL*/);
int sr_jfa_update(int K, int D, int R, const double *A, const double *C, double *W /*in: old, out: new*/, int64_t *skipped /*or NULL*/);
int sr_jfa_train(SRJfa *h, double *W /*in/out*/, int R, int n_iter, double *y /*[G][R] or NULL*/, int64_t *skipped /*or NULL*/);
void sr_jfa_close(SRJfa *h);
int sr_jfa_plan(int64_t G, int K, int D, int R, int64_t scratch_bytes, int lds_rows, int n_cu, int64_t *out, int n_out);

/* ---- JFA trial scoring (csrc/jfa_score.hip): the score matrix out [J][T] of J models (speaker factors y [J][Ry], z [J][K*D]) against
 * T test segments (raw statistics N [T][K], F [T][K*D], F NOT centred), by the reference's two scorers (src/jfa/; MATLAB there, a
 * loop over segments and models), float64 throughout, in one batched call.  d [K*D] and z may be NULL: zeros.
 * sr_jfa_score_integrated (kscore_famous_19.m: the channel factors integrated out).  M_0 = m, M_j = m + z_j .* d + y_j v:
 *   lin[t][j]  = sum_i F[t][i] M_j[i] / E[i]        quad[t][j] = sum_c N[t][c] sum_d M_j[c,d]^2 / E[c,d]
 *   L_t = I + sum_c N[t][c] u_c diag(1 / E_c) u_c^T a_t = u (F[t] ./ E)        h[t][j] = sum_c N[t][c] u_c (M_j,c ./ E_c)
 *   quad2 = || chol(L_t)^-1 (a_t - h[t][j]) ||^2    s = (lin - quad / 2 + quad2 / 2) / n_t,  n_t = sum_c N[t][c]
 *   out[j-1][t] = s[t][j] - s[t][0]
 *   u_c (M_j,c ./ E_c) is formed once per call for every (mixture, model), so h of all pairs is one product over K: K Ru operations a
 *   pair where the reference spends K D Ru.  One workgroup per segment factors L_t and runs ONE forward substitution over all J + 1
 *   right-hand sides.  The reference leaves the UBM's score un-subtracted where a score is exactly 0; that is not reproduced.
 * sr_jfa_score_linear (linear_scoring.m), with the segments' channel factors x [T][Ru]:
 *   out[j][t] = sum_i ((z_j .* d + y_j v)[i] / E[i]) (F[t][i] - N[t][c(i)] (m + x_t u)[i]) / n_t
 * The test segments run in chunks whose blocks (Ru^2 + (J + 1) Ru doubles a segment) fit "jfa_scratch_mib"; "jfa_lds_rows" chooses the
 * factorisation path as for sr_jfa_factors.  No atomics: a (model, segment) score is the same bits for the segment alone or in any
 * batch, for the model alone or in any model set, under any bound, on either path's chunking, from run to run.
 * mask (or NULL): uint8 [mask_rows][mask_cols], which must be [J][T]; where it is 0 the score is 0.0 exactly.  A segment with
 * n_t = 0 gets zeros and is counted in empty_segments (the reference divides by zero there); a segment whose L_t does not factor (a
 * pivot <= 0 or not finite: impossible short of overflow) gets zeros and is counted in bad_segments.  The counters may be NULL.
 * Refused, before the device is touched, with a message that names the remedy: T, J, K, D, Ry or Ru < 1, Ry or Ru above 512, a
 * non-finite value in any input, a negative N, E <= 0, linear mode without x, a mask of another shape, a scratch bound below one
 * segment's blocks.  Refused in a process forked after the GPU runtime was initialised.
 * Timer kinds (none is added): SR_T_JFA_GRAM the scalings, P, the cross kernel and the elementwise synthesis / compensation;
 * SR_T_JFA_GEMM_L L; SR_T_JFA_GEMM_B the reductions over K * D (a, lin, the linear score matrix); SR_T_JFA_GEMM_A the reductions over
 * K (quad, h); SR_T_JFA_GEMM_C the synthesis products y v and x u; SR_T_JFA_FACTOR the factorisation, substitution and scores.
 * sr_jfa_score_plan: what such a call decides (csrc/jfa_plan.cpp; host only when n_cu > 0), for tests; mode 0 integrated, 1 linear.
 * Writes 56 fields (n_out >= 56) and returns 56, -1 on refusal: mode, segments per chunk, chunks, a segment's bytes inside the bound,
 * a chunk's; bytes of M, M ./ E, u (with u ./ E), P, q, G, N, F, lin, quad, a, out and linear mode's compensated statistics; the
 * factorisation path and the largest Ru of the LDS path; the grids of the y v product, the synthesis, the two scalings, the gram and
 * cross (x, y, z) kernels, the L, a, lin, quad and h products, the scoring kernel, linear mode's x u product, compensation and score
 * product; LDS bytes of the gram, GEMM, cross and scoring kernels; rounds of a chunk's scoring launch over the chip; the built limits
 * of Ry / Ru, of the LDS path and of J; 0, 0. */
int sr_jfa_score_integrated(int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *N /*[T][K]*/, const double *F /*[T][K*D]*/,
                            const double *m /*[K*D]*/, const double *E /*[K*D]*/, const double *d /*[K*D] or NULL*/, const double *v /*[Ry][K*D]*/,
                            const double *u /*[Ru][K*D]*/, const double *z /*[J][K*D] or NULL*/, const double *y /*[J][Ry]*/,
                            const unsigned char *mask /*or NULL*/, int64_t mask_rows, int64_t mask_cols, double *out /*[J][T]*/,
                            int64_t *empty_segments /*or NULL*/, int64_t *bad_segments /*or NULL*/);
int sr_jfa_score_linear(int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *N, const double *F, const double *m, const double *E,
                        const double *d /*or NULL*/, const double *v, const double *u, const double *z /*or NULL*/, const double *y,
                        const double *x /*[T][Ru]*/, const unsigned char *mask /*or NULL*/, int64_t mask_rows, int64_t mask_cols,
                        double *out /*[J][T]*/, int64_t *empty_segments /*or NULL*/);
int sr_jfa_score_plan(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, int lds_rows, int n_cu, int64_t *out,
                      int n_out);

/* ---- The JFA leg resident on the device (csrc/jfa_stats.hip): statistics that stay there from the Baum-Welch pass to the score
 * matrix.  Nothing above changes; these are the same kernels reached without the statistics going home in between.
 * SRStats: raw N [n][K] and F [n][K*D] (not centred, mixture-major, float64) of n sessions on one device.
 * sr_bw_stats_resident: the passes of sr_bw_stats_batch -- same plan, same kernels, same launch order -- with the reduce writing
 *   into buffers the handle owns; only ll and dropped come back.  sr_stats_get of the handle returns the bits sr_bw_stats_batch
 *   returns.  The result is checked by a small device kernel (finite, N >= 0) when the handle is made.  At least one utterance.
 * sr_stats_from_host: uploads host arrays once, validated first (finite values, N >= 0: the texts of sr_jfa_open).
 * sr_stats_info: 4 fields (n_out >= 4): n, K, D, device; returns 4.  sr_stats_get: N and / or F back to the host.
 * sr_stats_take: a new handle of the rows named, a device gather: any order, repeats allowed.
 * sr_stats_close: NULL and a handle closed before are harmless; every other call refuses a closed handle by its text.
 * sr_jfa_open_centred: the grouping and centring on the device into an ordinary SRJfa (sr_jfa_factors, sr_jfa_train, sr_jfa_close
 *   work on it unchanged; it owns its arrays: the statistics handle may be closed while it lives).  ids [n]: 0-based labels below
 *   n_labels; N_j (x) w: the row of K counts expanded over D.
 *     mode 0, groups = the labels that occur, ascending:  N_g = sum_{j in g} N_j,
 *             Fc_g = sum_{j in g} (F_j - N_j (x) (x_j u)) - N_g (x) (m + z_g .* d + y_g v)
 *     mode 1, groups = sessions:  Fc_j = (F_j - N_j (x) (x_j u)) - N_j (x) (m + z_s .* d + y_s v),  s = ids[j]
 *   A NULL pair (d and z [n_labels][K*D]; v [Ry][K*D] and y [n_labels][Ry]; u [Ru][K*D] and x [n][Ru]) is an absent term, not a
 *   product with zeros.  y v and x u run on v_mfma_f64_16x16x4_f64 through the GEMM kernel of sr_jfa_factors, x u a chunk of
 *   sessions at a time under "jfa_scratch_mib" (chunks are a function of n, K*D and the bound only); one streaming kernel reads F,
 *   N and the product once and writes Fc once.  A group's sessions are added in ascending session order, N_g with plain adds; no
 *   atomics: a group's row is the same bits alone (its sessions taken into a handle of their own), inside any batch, under any
 *   bound, from run to run.
 * sr_jfa_statistics: what a factor handle holds, N [G][K] and / or Fc [G][K*D].
 * sr_jfa_centre_plan: what sr_jfa_open_centred decides (csrc/jfa_plan.cpp, host only; Ry / Ru 0: the term is absent), for tests.
 *   Writes 16 fields (n_out >= 16) and returns 16, -1 on refusal: mode, sessions per chunk, chunks, bytes of a chunk's product,
 *   bounds of the bytes of N, Fc, y v and z, doubles per lane of the centring kernel, the grids x y of a chunk's x u product, of
 *   y v and of the centring kernel, the GEMM's row tile (chunks but the last are multiples of it).
 * sr_jfa_zd: estimate_z_and_d.m on a handle's resident N_g, Fc_g and E (from sr_jfa_open_centred centred with y and x, or from
 *   sr_jfa_open):  L = 1 + N_g (x) d^2 / E,  z = Fc_g .* d ./ (E .* L),  a = sum_g (1 / L + z^2) .* N_g,  b = sum_g z .* Fc_g,
 *   d <- b / a, n_iter times in ONE launch (columns do not interact; the sums run in group order).  d in / out (n_iter = 0: one
 *   evaluation, d untouched); z, a, b (each or NULL): of the last round, i.e. for the d that round started from.  A column no
 *   group occupies with d = 0 gives 0 / 0 as the reference does.
 * sr_jfa_score_integrated_stats / sr_jfa_score_linear_stats: the two scorers with a statistics handle in place of T, K, D, N, F:
 *   the same launches on the handle's buffers; n_t and the empty-segment count come from a device kernel that adds a segment's K
 *   counts in mixture order -- the scores are the same bits as the host-array entries give for the same numbers.
 * Timer kinds (none is added): SR_T_JFA_GRAM the check, gather, group-count, centring, z / d and n_t kernels; SR_T_JFA_GEMM_C y v, x u.
 * Refused, before the device is touched, with a message that names the argument and the remedy: a NULL or closed statistics
 * handle, labels that are negative or >= n_labels, Ry / Ru outside 1 .. 512, a non-finite value in any host array, E <= 0, half
 * of a pair, rows outside the handle, a bound below one chunk of 64 sessions, a handle on another device than the calling
 * thread's; and in a process forked after the GPU runtime was initialised. */
typedef struct SRStats SRStats;
SRStats *sr_bw_stats_resident(SRModelSet *set, int model, SRBatch *feats, double *ll /*[U] or NULL*/, int64_t *dropped /*[U] or NULL*/);
SRStats *sr_stats_from_host(int64_t n, int K, int D, const double *N /*[n][K]*/, const double *F /*[n][K*D]*/);
int sr_stats_info(const SRStats *s, int64_t *out /*n, K, D, device*/, int n_out);
int sr_stats_get(const SRStats *s, double *N /*or NULL*/, double *F /*or NULL*/);
SRStats *sr_stats_take(const SRStats *s, const int64_t *rows, int64_t n_rows);
void sr_stats_close(SRStats *s);
SRJfa *sr_jfa_open_centred(const SRStats *s, const double *E /*[K*D]*/, const double *m /*[K*D]*/, int mode, const int64_t *ids /*[n]*/,
                           int64_t n_labels, const double *d /*[K*D] or NULL*/, const double *z /*[n_labels][K*D] or NULL*/,
                           const double *v /*[Ry][K*D] or NULL*/, int Ry, const double *y /*[n_labels][Ry] or NULL*/,
                           const double *u /*[Ru][K*D] or NULL*/, int Ru, const double *x /*[n][Ru] or NULL*/);
int sr_jfa_statistics(SRJfa *h, double *N /*[G][K] or NULL*/, double *Fc /*[G][K*D] or NULL*/);
int sr_jfa_centre_plan(int64_t n, int64_t n_labels, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, int64_t *out, int n_out);
int sr_jfa_zd(SRJfa *h, double *d /*[K*D] in/out*/, int n_iter, double *z /*[G][K*D] or NULL*/, double *a /*[K*D] or NULL*/,
              double *b /*[K*D] or NULL*/);
int sr_jfa_score_integrated_stats(const SRStats *tst, int64_t J, int Ry, int Ru, const double *m, const double *E, const double *d /*or NULL*/,
                                  const double *v, const double *u, const double *z /*or NULL*/, const double *y,
                                  const unsigned char *mask /*or NULL*/, int64_t mask_rows, int64_t mask_cols, double *out /*[J][T]*/,
                                  int64_t *empty_segments /*or NULL*/, int64_t *bad_segments /*or NULL*/);
int sr_jfa_score_linear_stats(const SRStats *tst, int64_t J, int Ry, int Ru, const double *m, const double *E, const double *d /*or NULL*/,
                              const double *v, const double *u, const double *z /*or NULL*/, const double *y, const double *x /*[T][Ru]*/,
                              const unsigned char *mask /*or NULL*/, int64_t mask_rows, int64_t mask_cols, double *out /*[J][T]*/,
                              int64_t *empty_segments /*or NULL*/);

/* ---- Score normalisation (csrc/score_norm.hip, csrc/norm_plan.cpp): a score matrix S [J][T] (models x test segments) normalised
 * against impostor cohorts on the device, float64 throughout, row-major.  Ez [J][Cz]: the models against the Z-cohort (impostor
 * segments); Tt [Ct][T]: the T-cohort models against the test segments; Zt [Ct][Cz]: the T-cohort models against the Z-cohort.  A
 * matrix the mode does not read is NULL (its cohort size is ignored).  mu / sigma: the mean and the population standard deviation
 * (ddof = 0); "top-N of a row": the N largest values, ties to the lower index, -0.0 taken as +0.0.  mode:
 *   0 z    (S - mu(Ez[j,:])) / sigma(Ez[j,:])                 1 t    (S - mu(Tt[:,t])) / sigma(Tt[:,t])
 *   2 zt   S' = z-norm of S by Ez; Tt' = z-norm of Tt by Zt, row c of Tt by row c of Zt; out = t-norm of S' by Tt'
 *   3 s    (z + t) / 2                                        4 as1  as s, the moments over the top-N of Ez[j,:] and of Tt[:,t]
 *   5 as2  Cz = Ct = C, cohort member c both a segment and a model; I_t = the top-N of Tt[:,t], I_j = the top-N of Ez[j,:]:
 *          ((S - mu(Ez[j,I_t])) / sigma(Ez[j,I_t]) + (S - mu(Tt[I_j,t])) / sigma(Tt[I_j,t])) / 2
 * top_n >= 2 in the adaptive modes (ignored in the others); top_n >= C selects everything.
 * THE BUILT LIMIT: a cohort of at most 16384 members (Cz, Ct, C <= 16384): norm_select_moments_kernel keeps a cohort row in LDS as 64-bit
 * keys next to its 256-bin histogram, 128 KiB + 1 KiB + 96 B of a gfx950 compute unit's 160 KiB.  At most 65535 * 64 models or test
 * segments and 2^36 trials a call.
 * One workgroup per cohort row finds the N-th largest value by radix select on the order-preserving 64-bit key of the double (eight
 * 8-bit passes over an LDS histogram, no sort), resolves ties at the threshold by a prefix count in index order, and sums the moments
 * of the selected values in an order that depends on the selected set only; a column of Tt is read with stride T.  as2's sums over
 * the other side's selection are four products on v_mfma_f64_16x16x4_f64 through the GEMM kernel of sr_jfa_factors:
 * Es SelT^T, (Es .* Es) SelT^T, SelE Ts, SelE (Ts .* Ts), with SelT [T][C] / SelE [J][C] the 0/1 selections and Es = Ez - mu(Ez[j,:]),
 * Ts = Tt - mu(Tt[:,t]) shifted by the full row's / column's mean.  A pair whose variance the products cannot tell from 0 (not above
 * 2^-30 of the mean square about the shift: a selected set that is constant, or nearly, in a row that is not) takes its moments from
 * the selected values themselves, relative to the first of them, so that a constant set is degenerate exactly.  That scratch lives under "norm_scratch_mib": the test segments run
 * in chunks that fit.  No atomics on global memory and no float atomics: a score is the same bits under any bound and from run to run;
 * a row's selection and moments are the same bits alone and in any batch.
 * Degenerate pairs: a moment pair whose variance is not > 0 or not finite (a constant cohort row; a cohort of one).  Every trial that
 * needs it gets 0.0 exactly; no NaN is ever written.  degenerate (or NULL) [2]: the pairs of the enrolment side (Ez) and of the test
 * side (Tt; in zt the columns of Tt' plus the rows of Zt, whose rows of Tt' are zeros) -- rows / columns in modes 0 .. 4, (model,
 * segment) pairs in as2.
 * sr_score_norm_select: the selection stage alone on X [rows][C]: idx [rows][min(top_n, C)] the selected indices of each row,
 * ascending, mu / sigma [rows] the moments of the selected values (sigma 0.0: degenerate).  Each output may be NULL.
 * sr_score_norm_plan: what a call decides (csrc/norm_plan.cpp; host only when n_cu > 0), for tests.  Writes 40 fields (n_out >= 40)
 * and returns 40, -1 on refusal: mode, values per moment pair on the enrolment and on the test side, test segments per chunk, chunks;
 * as2's bytes inside the bound: once per call (3 J C doubles), per test segment (3 C + 4 J doubles), of a full chunk with the fixed
 * part; bytes of S, Ez, Tt, Zt, out, the moments with their flags, zt's Tt', as2's counters; workgroups of the selection over Ez, over
 * a chunk of Tt, over Zt; its LDS bytes on either side; the grids of the two shifted copies, of the products Es SelT^T (x, y) and
 * SelE Ts (x, y), the GEMM's LDS bytes, the apply kernel's grid (x = models, y = blocks of 256 segments); rounds of the largest
 * selection launch over the chip; the built limits of C and of J / T; lanes per workgroup; six zeros.
 * Refused, before the device is touched, with a message that names the argument and the remedy: a mode outside 0 .. 5, J or T < 1 or
 * above the limits, a cohort of no members or above the built limit, top_n < 2 in an adaptive mode, as2 with Cz != Ct, a matrix the
 * mode needs missing, a non-finite value anywhere, a bound below one chunk.  Refused in a process forked after the GPU runtime was
 * initialised.
 * Timer kinds (none is added): SR_T_JFA_FACTOR the selection kernel; SR_T_JFA_GRAM the shifted copies; SR_T_JFA_GEMM_A the two products
 * with SelT; SR_T_JFA_GEMM_B the two with SelE; SR_T_JFA_UPDATE the apply kernel. */
int sr_score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S /*[J][T]*/, const double *Ez /*[J][Cz] or NULL*/,
                  const double *Tt /*[Ct][T] or NULL*/, const double *Zt /*[Ct][Cz] or NULL*/, double *out /*[J][T]*/,
                  int64_t *degenerate /*[2] or NULL*/);
int sr_score_norm_select(int64_t rows, int64_t C, int top_n, const double *X /*[rows][C]*/, int64_t *idx /*[rows][min(top_n,C)] or NULL*/,
                         double *mu /*[rows] or NULL*/, double *sigma /*[rows] or NULL*/);
int sr_score_norm_plan(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, int64_t scratch_bytes, int n_cu, int64_t *out,
                       int n_out);

/* ---- The i-vector back end (csrc/plda.hip, csrc/plda_plan.cpp): what follows i-vector extraction (sr_jfa_factors with one group per
 * session and the total-variability matrix as W), on the device, float64 throughout, row-major, vectors of 1 <= R <= 512 dimensions.
 * sr_backend_fit: kind 0 (whiten): mu [R] the mean of the rows of X [n][R] and A [R][R] = chol(Sigma)^-1, Sigma the total covariance
 *   (ddof = 0), so that (X - mu) A^T has covariance I; kind 1 (wccn): A = chol(W)^-1, W the within-class covariance of the rows about
 *   the means of their classes ids [n] in 0 .. n_labels - 1.  A is lower triangular.  A covariance that does not factor is refused.
 * sr_backend_apply: Y [n][R] = (X - mu) A^T; with length_norm != 0 every row scaled to unit 2-norm, a row whose norm is 0 or not finite
 *   becoming exact zeros and counted in zero_rows (or NULL).
 * sr_cosine_score: out [J][T] = <e_j, x_t> / (|e_j| |x_t|): one product and the row norms; a pair with a norm of 0 scores 0.0.
 * Two-covariance Gaussian PLDA: x_ij = mu + y_i + e_ij, y ~ N(0, Sb), e ~ N(0, Sw), Sb and Sw full [R][R].
 * sr_plda_train: n_iter EM rounds on X [n][R] with 0-based speaker labels ids [n] (every label 0 .. n_labels - 1 occurs), from the Sb
 *   and Sw given (default_start 0), or with both starting from half the total covariance T2 / (2 n) formed on the device
 *   (default_start 1: what Sb and Sw hold is not read); they receive the result.  mu [R] (or NULL) receives the mean of the rows,
 *   formed once in row order.  Per round, with
 *   n_i the rows of speaker i, f_i the sum of its centred rows, T2 the scatter of all centred rows:
 *     Phi_c = (Sb^-1 + c Sw^-1)^-1 per distinct count c      yhat_i = Phi_{n_i} Sw^-1 f_i      Sb <- (sum_i Phi_{n_i} + Yhat^T Yhat) / S
 *     Sw <- (T2 - F^T Yhat - Yhat^T F + Yhat^T diag(n_i) Yhat + sum_i n_i Phi_{n_i}) / n
 *   The speakers are sorted by count, so a count class is a contiguous row range: one factorisation and one inverse per distinct count
 *   per round.  n_iter rounds in one call give the bits of n_iter calls of one round.  iterations / n_classes / stop (each or NULL):
 *   the rounds done, the distinct counts, and why the rounds ended: 0 all ran, 1 Sb did not factor, 2 Sw did not, 3 a Sb^-1 + c Sw^-1
 *   did not, 4 a round produced a non-finite value.  On 1 .. 4 Sb and Sw hold the last pair that factored (the input pair when the
 *   first round stops) and `iterations` says which; no NaN reaches the outputs.  The pair the LAST round returns is checked for
 *   finite values only, not factored: stop 0 does not promise that a further call, or sr_plda_score, can factor it -- that call
 *   says so itself (iterations 0 and a stop code; bad_classes).
 * sr_plda_score: out [J][T], the log-likelihood ratio of "segment t is of model j's speaker" against "of another"; model j has
 *   enrol_n[j] >= 1 enrolment vectors whose raw sum is E[j] ([J][R]); X [T][R] the test vectors.  With c = enrol_n[j],
 *   yhat_j = Phi_c Sw^-1 (E[j] - c mu), P_c = (Phi_c + Sw)^-1, P_0 = (Sb + Sw)^-1, x = x_t - mu:
 *     out[j][t] = -1/2 ln det(Phi_c + Sw) - 1/2 (x - yhat_j)^T P_c (x - yhat_j) + 1/2 ln det(Sb + Sw) + 1/2 x^T P_0 x
 *   The cross term Yhat_c P_c X^T is one product per distinct count straight into the output's rows; the test segments run in chunks
 *   under "plda_scratch_mib".  A score is the same bits for its model alone, its segment alone, in any batch and under any bound.
 *   A count class whose blocks do not factor gets exact zeros in its rows and is counted in bad_classes (or NULL).
 *   Outside the bound, growing with the number nc of DISTINCT counts (at most J): a Phi_c and a P_c per count, (3 nc + 6) R^2 doubles
 *   with the factorisation's scratch, and one X P_c product over all T segments per count -- 2 T R^2 operations each against the
 *   cross term's 2 J T R in all.  A trial list with many distinct counts pays for each; enrol_mode "average" has one.
 * sr_plda_plan: what a call decides (csrc/plda_plan.cpp; host only when n_cu > 0), for tests.  kind 0: training, counts = ids [rows],
 *   groups = n_labels; kind 1: scoring, counts = enrol_n [rows], groups ignored.  Writes 36 fields (n_out >= 36) and returns 36, -1 on
 *   refusal: kind, R, rows, groups, T, distinct counts, vectors per launch of T2's sum and the launches, speakers per launch of the
 *   sums over speakers and the launches, test segments per chunk and the chunks, bytes per segment and of a full chunk inside the
 *   bound, bytes of the R x R blocks and of the row arrays, the factorisation path (0 LDS, 1 global memory) and the largest R of the
 *   LDS path, the factorisation's and the GEMM's LDS bytes, the grids of the centring (x), the class sums (x, y), the factorisations
 *   (x), the widest row product (x, y), the R x R sums (x, y), the row dot products (x), the cross term (x, y), the assembly (x), the
 *   factorisation's rounds over the chip, the built limits of R and of the rows, the column groups (of four) of the factor's
 *   inverse on the global-memory path (0 on the LDS path).  perm (or NULL) [groups]: sorted position -> label or model;
 *   classes (or NULL) [3 * groups]: (count, first sorted position, size) of every class, ascending count.
 * Refused, before the device is touched, with a message that names the argument and the remedy: R < 1 or R > 512; n, J or T < 1 or
 * above 65535 * 64; a label out of range or without a row; a non-finite input; enrol_n < 1; an Sb or Sw that is not symmetric; a
 * bound below one chunk.  Refused in a process forked after the GPU runtime was initialised.
 * Timer kinds (none is added): SR_T_JFA_GRAM the elementwise kernels, the class sums and the row dot products; SR_T_JFA_FACTOR the
 * factorisations; SR_T_JFA_GEMM_B the products with Sw^-1, P_c and A; SR_T_JFA_GEMM_L those with Phi_c and Yhat P_c; SR_T_JFA_GEMM_A
 * the sums over vectors and speakers; SR_T_JFA_GEMM_C the cross term and the cosine's product; SR_T_JFA_UPDATE the new covariances,
 * the length normalisation and the score assembly. */
int sr_backend_fit(int kind, int64_t n, int R, const double *X /*[n][R]*/, const int64_t *ids /*[n], wccn; else NULL*/, int64_t n_labels,
                   double *mu /*[R]*/, double *A /*[R][R]*/);
int sr_backend_apply(int64_t n, int R, const double *X /*[n][R]*/, const double *mu /*[R]*/, const double *A /*[R][R]*/, int length_norm,
                     double *Y /*[n][R]*/, int64_t *zero_rows /*or NULL*/);
int sr_cosine_score(int64_t J, int64_t T, int R, const double *E /*[J][R]*/, const double *X /*[T][R]*/, double *out /*[J][T]*/);
int sr_plda_train(int64_t n, int R, const double *X /*[n][R]*/, const int64_t *ids /*[n]*/, int64_t n_labels, int n_iter, int default_start,
                  double *mu /*[R] or NULL*/, double *Sb /*[R][R] in/out*/, double *Sw /*[R][R] in/out*/, int *iterations /*or NULL*/,
                  int *n_classes /*or NULL*/, int *stop /*or NULL*/);
int sr_plda_score(int64_t J, int64_t T, int R, const double *mu /*[R]*/, const double *Sb /*[R][R]*/, const double *Sw /*[R][R]*/,
                  const double *E /*[J][R]*/, const int64_t *enrol_n /*[J]*/, const double *X /*[T][R]*/, double *out /*[J][T]*/,
                  int64_t *bad_classes /*or NULL*/);
int sr_plda_plan(int kind, int R, int64_t rows, int64_t groups, int64_t T, const int64_t *counts /*[rows]*/, int64_t scratch_bytes, int lds_rows,
                 int n_cu, int64_t *out, int n_out, int64_t *perm /*[groups] or NULL*/, int64_t *classes /*[3 * groups] or NULL*/);

/* ---- The symmetric eigen-solver and what the i-vector back end builds on it (csrc/eig.hip, csrc/eig_plan.cpp, csrc/backend_eig.hip):
 * LDA and PLDA scoring with the model diagonalised once.  On the device, float64 throughout, row-major, 1 <= R <= 512.
 * sr_sym_eig: A [R][R] symmetric (the lower triangle is read; not assumed definite) -> w [R] DESCENDING and V [R][R], column k the unit
 *   eigenvector of w[k].  Signs: every vector's component of largest magnitude is positive, the lowest index winning a tie.  Two-sided
 *   block Jacobi: blocks of 32 columns (an odd number padded with an empty phantom block), a sweep the blocks - 1 rounds of the
 *   round-robin tournament, a round three launches (the pairs' 64 x 64 sub-problems by cyclic Jacobi rotations in LDS, the column
 *   update of A and V, the row update of A); R <= 64 is one launch.  Stops when the largest off-diagonal magnitude is
 *   <= R 2^-52 max|A|, or at the cap of 40 sweeps.  sweeps / converged (each or NULL): the sweeps taken; 1, or 0 when the cap was
 *   reached -- w and V then hold what there is, and the return value is still 0.  The same bits from run to run.
 * sr_gen_eig: Sb v = psi Sw v for symmetric Sb and positive definite Sw [R][R]: L = chol(Sw), M = L^-1 Sb L^-T (symmetrised),
 *   M = Q diag(psi) Q^T by the solver above, V = L^-T Q, so that V^T Sw V = I and V^T Sb V = diag(psi), psi [R] descending, the signs
 *   those of Q.  status (or NULL): 0 ok; 1 Sw did not factor: psi and V are exact zeros; 2 the sweep cap was reached.
 * sr_lda_fit: X [n][R] with 0-based class labels ids [n] (every label 0 .. n_labels - 1 occurs) -> mu [R] the mean of the rows (formed
 *   in row order), and with Sw the within-class covariance about the class means (ddof 0, what sr_backend_fit kind 1 factors) and
 *   Sb = (1 / n) sum_i n_i (m_i - mu)(m_i - mu)^T (so that Sb + Sw is the total covariance): A [P][R] the first P generalised
 *   eigenvectors, as rows, and psi [P] their values, descending.  A Sw A^T = I_P: the projection arrives WCCN-normalised.
 *   1 <= P <= min(R, n_labels - 1).  An Sw that does not factor is refused as sr_backend_fit refuses it.
 * sr_backend_project: Y [n][P] = (X - mu) A^T for A [P][R], 1 <= P <= R; with length_norm != 0 every row scaled to unit 2-norm, a row
 *   whose norm is 0 or not finite becoming exact zeros and counted in zero_rows (or NULL), as sr_backend_apply does.
 * sr_plda_score_diag: sr_plda_score's result from the model diagonalised: mu [R], V [R][R] and psi [R] of sr_gen_eig(Sb, Sw); E,
 *   enrol_n, X, out, bad_classes as sr_plda_score takes them.  With u_t = V^T (x_t - mu), G_j = V^T (E[j] - c mu), c = enrol_n[j],
 *   h_cd = psi_d / (c psi_d + 1), s_cd = 1 + h_cd, s_0d = 1 + psi_d, m_jd = h_cd G_jd:
 *     out[j][t] = -1/2 sum_d ln s_cd - 1/2 (sum_d u_td^2 / s_cd - 2 sum_d (m_jd / s_cd) u_td + sum_d m_jd^2 / s_cd)
 *                 + 1/2 sum_d ln s_0d + 1/2 sum_d u_td^2 / s_0d
 *   No factorisation: two products with V, ONE cross product over all models whatever their counts, one product U.^2 [T][R] by
 *   [R][classes + 1]; the segments run in chunks under "plda_scratch_mib" (2 R + classes + 1 doubles a segment).  The same bits for a
 *   model alone, a segment alone, in any batch, under any bound.  A psi that is not finite or below -1e-9 of the largest magnitude
 *   zeroes and counts every class; a class with a (c + 1) psi_d + 1 <= 0 -- its s_cd would not be positive; c psi_d + 1 <= 0 is
 *   among these -- is zeroed and counted (a backstop behind the first rule: it can only be met by a psi whose largest magnitude is
 *   above 1e9 / (c + 1)).  No NaN is written.
 * sr_eig_plan: what sr_sym_eig decides (csrc/eig_plan.cpp; host only when n_cu > 0), for tests.  Writes 24 fields (n_out >= 24) and
 *   returns 24, -1 on refusal: R, the block width b, the blocks, 1 with a phantom block, the rounds of a sweep, the pairs of a round
 *   (the phantom's included), 1 on the single-launch path (R <= 2 b: no rounds), the sweep cap, the cap of a pair's inner sweeps,
 *   the LDS bytes of the solve and of the update stages, the grid of the solve stage (the working pairs), of the column stage (x, y, z)
 *   and of the row stage (x, y), the launches of a sweep, the bytes of the working arrays, the rounds the widest launch makes over
 *   the chip, the built limit of R, the rows of an update tile, 2 b, the lanes of a workgroup.  schedule (or NULL)
 *   [rounds][pairs][2]: the block pairs (p < q) of every round; q == blocks names the phantom: that pair does no work.
 * Refused, before the device is touched, with a message that names the argument and the remedy: R < 1 or R > 512; a null argument; a
 * non-finite value; a matrix that is not symmetric (sr_plda_score's rule); P out of range; the label and row errors of
 * sr_backend_fit; enrol_n < 1; a bound below one chunk.  Refused in a process forked after the GPU runtime was initialised.
 * Timer kinds (none is added): SR_T_JFA_FACTOR the solver's launches and the Cholesky; SR_T_JFA_GEMM_C every product of these calls;
 * SR_T_JFA_GEMM_A the covariance sums of sr_lda_fit; SR_T_JFA_GRAM the centring, the class sums and the row dot products;
 * SR_T_JFA_UPDATE the elementwise kernels, the length normalisation and the score assembly. */
int sr_sym_eig(int R, const double *A /*[R][R]*/, double *w /*[R]*/, double *V /*[R][R]*/, int *sweeps /*or NULL*/, int *converged /*or NULL*/);
int sr_gen_eig(int R, const double *Sb /*[R][R]*/, const double *Sw /*[R][R]*/, double *psi /*[R]*/, double *V /*[R][R]*/, int *sweeps /*or NULL*/,
               int *status /*or NULL*/);
int sr_lda_fit(int64_t n, int R, const double *X /*[n][R]*/, const int64_t *ids /*[n]*/, int64_t n_labels, int P, double *mu /*[R]*/,
               double *A /*[P][R]*/, double *psi /*[P]*/);
int sr_backend_project(int64_t n, int R, int P, const double *X /*[n][R]*/, const double *mu /*[R]*/, const double *A /*[P][R]*/, int length_norm,
                       double *Y /*[n][P]*/, int64_t *zero_rows /*or NULL*/);
int sr_plda_score_diag(int64_t J, int64_t T, int R, const double *mu /*[R]*/, const double *V /*[R][R]*/, const double *psi /*[R]*/,
                       const double *E /*[J][R]*/, const int64_t *enrol_n /*[J]*/, const double *X /*[T][R]*/, double *out /*[J][T]*/,
                       int64_t *bad_classes /*or NULL*/);
int sr_eig_plan(int R, int n_cu, int64_t *out, int n_out, int *schedule /*[rounds][pairs][2] or NULL*/);

/* ---- Score calibration and fusion (csrc/calib.hip, csrc/calib_plan.cpp): prior-weighted linear logistic regression (Bruemmer's FoCal /
 * BOSARIS) that turns the scores of a verification run into log-likelihood ratios, its objective Cllr, and the error counts behind the
 * actual DCF.  On the device, float64 throughout.
 *   X [S][n] row-major: X[s][i] is system s's score for trial i (a quality measure such as a duration is one more row).
 *   lab [n] int8: 1 target, 0 non-target, any negative value "not a trial" -- skipped everywhere and counted; its scores may hold
 *   anything (NaN included): they are replaced by a select and never enter the arithmetic.
 *   theta = (w_1 .. w_S, b);  z_i = sum_s w_s X[s][i] + b;  tau = ln(P / (1 - P));  sp(a) = max(a, 0) + log1p(exp(-|a|));
 *   f(theta) = (1 / ln 2) [P / n_t sum_tar sp(-(z_i + tau)) + (1 - P) / n_n sum_non sp(z_i + tau)] + lam / 2 sum_s w_s^2
 *   with a_i = (X[0][i], .., X[S-1][i], 1), s_i = 1 / (1 + exp(-(z_i + tau))), c_i = P / n_t for targets, (1 - P) / n_n for non-targets:
 *   g = (1 / ln 2) sum_i c_i (s_i - [target]) a_i + lam (w, 0),  H = (1 / ln 2) sum_i c_i s_i (1 - s_i) a_i a_i^T + lam diag(1 .. 1, 0).
 *   The ridge lam is on the S weights only.  Cllr(llr, lab) is f at S = 1, theta = (1, 0), P = 0.5, lam = 0.
 * THE BUILT LIMIT: up to 8 systems (S <= 8): calib_pass_kernel keeps f, g and the upper triangle of H, 55 float64 accumulators at S = 8,
 * in registers, one instance per S.  At most 2^35 trials a call, 16 thresholds a counts call.
 * sr_calib_train: damped Newton from theta0 (NULL: zeros).  A pass is one evaluation of (f, g, H): a workgroup of 256 lanes owns 4096
 *   consecutive trials, one exp per trial, a fixed summation tree, no atomics; a one-workgroup step kernel adds the blocks' sums in fixed
 *   order and takes the decisions:
 *     pass at theta0;  loop:  H = L L^T by Cholesky; a pivot not > 0 (not above 16 x 2^-52 of its diagonal element: the rounding of its
 *     own formation) or not finite -> stop SINGULAR;  d = -H^-1 g;  lam2 = -g^T d;  lam2 <= tol -> stop CONVERGED;  t = 1;  repeat: pass
 *     at theta + t d;  f_new finite and <= f -> accept, leave;  t /= 2;  t < 2^-20 -> stop STALLED;  a further pass needed with max_pass
 *     made -> stop CAP.
 *   Stop codes: 0 CONVERGED, 1 CAP, 2 SINGULAR, 3 STALLED.  theta is always the last accepted point and always finite.  Separable data
 *   with lam = 0 has no finite optimum: the call ends with whichever code it reaches; set a ridge.  The host enqueues pass + step up to
 *   max_pass (1 .. 1000) times and reads back the stop word alone, after every 4th pair.  The bits of a result depend on (X, lab, P,
 *   lam, theta0, tol, max_pass) only.
 *   state [sr_calib_plan's state length = 16 + 4 (S + 1) + (S + 1)(S + 2) / 2 doubles], written on return:  [0] the stop code, [1] phase,
 *   [2] passes, [3] accepted steps, [4] halvings, [5] f at theta, [6] t, [7] lam2, [8] n_t, [9] n_n, [10] skipped, [11] the pass cap,
 *   [12] S, [16 ..] theta [S + 1], the pending trial point [S + 1], d [S + 1], g [S + 1] and the upper triangle of H at theta.
 *   resume != 0: `state` is read first; it must come from a call with the same S and data that ended by CAP, and max_pass more passes
 *   are made (theta0 is ignored).  max_pass = a, then a resume with b, equals one call with a + b, bit for bit.
 * sr_calib_eval: one pass at theta -> f, g [S + 1] (or NULL), H [S + 1][S + 1] (or NULL).
 * sr_calib_apply: out[i] = z_i for all n (no labels: every position).  The same trial gives the same bits alone and in any batch.
 * sr_calib_counts: at m <= 16 thresholds thr (-inf and +inf allowed), with "accept iff llr >= thr": miss[j] the targets not accepted,
 *   fa[j] the non-targets accepted.  Integers per workgroup, added on the host: exact.
 * counts (or NULL) [3] of train / eval / counts: targets, non-targets, skipped.
 * sr_calib_plan: what a call decides (csrc/calib_plan.cpp; host only when n_cu > 0), for tests.  Writes 28 fields (n_out >= 28) and
 *   returns 28, -1 on refusal: S, n, the blocks of 4096 trials, the accumulators, the state length, the bytes of X, lab, the partial sums,
 *   the state, apply's out, the thresholds, the counters; the resident bytes of train / eval, of apply, of counts; the grids of the
 *   pass, step, apply and counts kernels; the rounds of the pass kernel over the chip; the built limits of S and of the thresholds;
 *   trials per block; lanes per workgroup; the pairs between two reads of the stop word; the
 *   built limits of max_pass and of n; a zero.  scratch_bytes > 0: refuse as a call under that bound would (call: 0 train, 1 apply, 2 counts).
 * The scores go up once per call and stay resident for every pass.  "calib_scratch_mib" (sr_set_option; 1 .. 2^20 MiB, default 8192)
 * bounds a call's resident bytes: a call above it is refused and told to raise the option or calibrate on fewer trials.
 * Refused, before the device is touched, with a message that names the argument and the remedy: S < 1 or S > 8; n < 1 or above the
 * limit; no target or no non-target; a label above 1; P not in (0, 1); lam < 0 or not finite; tol < 0; max_pass outside 1 .. 1000; a
 * non-finite score at a trial (skipped positions are not checked); a non-finite theta0 / theta; a NaN threshold; a null argument; a
 * state that cannot be resumed; resident bytes above the bound.  Refused in a process forked after the GPU runtime was initialised.
 * Timer kinds (none is added): SR_T_JFA_GEMM_A the pass kernel; SR_T_JFA_FACTOR the step kernel; SR_T_JFA_UPDATE apply and counts. */
int sr_calib_train(int S, int64_t n, const double *X /*[S][n]*/, const int8_t *lab /*[n]*/, double prior, double ridge, double tol, int max_pass,
                   const double *theta0 /*[S+1] or NULL*/, int resume, double *state /*[state length]*/, int64_t *counts /*[3] or NULL*/);
int sr_calib_eval(int S, int64_t n, const double *X /*[S][n]*/, const int8_t *lab /*[n]*/, double prior, double ridge, const double *theta /*[S+1]*/,
                  double *f, double *g /*[S+1] or NULL*/, double *H /*[S+1][S+1] or NULL*/, int64_t *counts /*[3] or NULL*/);
int sr_calib_apply(int S, int64_t n, const double *X /*[S][n]*/, const double *theta /*[S+1]*/, double *out /*[n]*/);
int sr_calib_counts(int64_t n, const double *llr /*[n]*/, const int8_t *lab /*[n]*/, int m, const double *thr /*[m]*/, int64_t *miss /*[m]*/,
                    int64_t *fa /*[m]*/, int64_t *counts /*[3] or NULL*/);
int sr_calib_plan(int S, int64_t n, int n_thr, int call, int64_t scratch_bytes, int n_cu, int64_t *out, int n_out);

/* ---- Who spoke when: windowed scores, the hold rule and a Viterbi decode on the device (csrc/timeline.hip) ----
 * A scoring pass's per-frame matrix [S][n_frames] (fp32, on the device) becomes a label per window of every recording of the batch.
 * Per recording of n frames, window W >= 1 and hop H >= 1 frames (independent of each other):
 *   windows   Nw = 0 if n = 0, else 1 + ceil(max(0, n - W) / H) (sr_timeline_windows); window j covers frames [j H, min(j H + W, n)),
 *             c_j of them (the last may be short).  With W < H that count can name a last window that starts at or behind frame n
 *             (the last frames lie in the gap between two windows); it is not formed: Nw = min(that, ceil(n / H)).
 *   sums      sum[j][s] = the float64 sum of the fp32 per-frame values of column s, added in frame order; q[j][s] = sum[j][s] / c_j in
 *             float64.  A NaN quotient becomes -inf before any comparison; the windows that had one are counted per recording.
 *   states    one per column.  bg >= 0: column bg is the "nobody" state, its emission q[j][bg] + threshold, its label -1; bg = -1: every
 *             column is a speaker.  Ties are broken everywhere in one order -- the speaker columns ascending, the nobody state last --
 *             and the first in that order wins.  A window whose best emission is -inf gets -1.
 *   mode 0    raw: the first maximum of the emissions in that order.
 *   mode 1    hold (the reference GUI's rule, gui.py:195-204): shown[0] = raw[0]; for j >= 1, if raw[j] != -1 and raw[j-1] != -1 and
 *             raw[j-1] != raw[j] then shown[j] = shown[j-1], else shown[j] = raw[j].  Each recording on its own.
 *   mode 2    viterbi: the path that maximises sum_j e_j(l_j) - beta (number of label changes), beta >= 0, every run but the last at
 *             least min_dur = m windows (1 .. 16).  Float64, states (s, k), k = 1 .. m:
 *               j = 0: d(s, 1) = e_0(s), every other state -inf.
 *               enter = max_s d_{j-1}(s, m) - beta, the first maximum in the order above.
 *               m = 1: d_j(s, 1) = e + max(d_{j-1}(s, 1), enter), staying wins equality.
 *               m >= 2: d_j(s, 1) = e + enter; d_j(s, k) = e + d_{j-1}(s, k - 1) for 1 < k < m;
 *                       d_j(s, m) = e + max(d_{j-1}(s, m), d_{j-1}(s, m - 1)), staying wins equality.
 *               end state: the first maximum over all (s, k), k from m down to 1 the major order, the order above the minor; labels
 *               by traceback.  Every operation is one float64 add or one compare ("a wins over b": a >= b), nothing is fused; the path
 *               score (d of the end state; 0 for an empty recording) is returned per recording.  Modes 0 and 1 return NaN there.
 *               Emissions of +inf are outside the contract (-inf + inf is a NaN in the recurrence).
 * sr_timeline_windows: Nw as above (0 for n <= 0, W < 1 or H < 1).  Host only.
 * sr_timeline_plan: what a call decides for S columns, min_dur and a recording of n_frames (csrc/timeline_plan.cpp; host only).
 *   Writes 16 fields (n_out >= 16) and returns 16, -1 on refusal: the windows; the forward kernel's variant (0: one wave, S <= 64;
 *   1: a lane per state, S <= 1024; 2: lanes loop over states, S <= 4096), its lanes, states per lane, the windows of emissions it
 *   holds ahead (the tile); the slots of the minimum-duration ring per state (m - 1; none for m <= 2), 1 when the ring sits in LDS, the
 *   forward kernel's LDS bytes; the frames a workgroup of the sum kernel spans at most (3 H + W), the frames it stages at a time, its
 *   LDS bytes, its grid (workgroups of four windows; blocks of 64 columns); back-pointer bytes per window (a stay bit per state in
 *   64-bit words + the entering state); the built limits of S (4096) and min_dur (16).
 * sr_timeline_decide: the decision on window sums in host memory -- upload, the decision kernels, one copy back; the direct test of
 *   those kernels.  sums[Nw_total][S], counts[Nw_total] (frames per window, >= 1), win_off[U + 1] (window offsets of the recordings,
 *   from 0).  label_out[Nw_total]; path_score_out[U] and bad_windows_out[U] may be NULL.
 * sr_timeline_batch: scores the feature batch (the per-frame matrix is the one sr_score_batch_set(frame_ll_out) returns for the same
 *   batch and flags, bit for bit: a saturated pass redone on the precise engines, the partial-product pairs patched), forms the window
 *   sums and decides.  win_off_out[U + 1] and label_out[Nw_total] are required (Nw_total from sr_timeline_windows over the batch's
 *   utterances); sums_out[Nw_total][S], path_score_out[U], bad_windows_out[U] may be NULL.  The call needs the memory frame_ll_out
 *   needs: S x n_frames floats on the device.
 * sr_fullset_timeline_batch: the same for a full-covariance set; every column is a speaker (bg = -1).
 * sr_timeline_pcm_batch: sr_mfcc_extract_batch (CMVN, nd orders of deltas) on resident PCM, then sr_timeline_batch; the features
 *   stay on the device.  Frame counts: sr_mfcc_num_frames.
 * The results are the same bits from run to run and do not depend on the recordings decided in the same call (no atomics).
 * Refused, before the device is touched, with the remedy: window < 1, hop < 1, min_dur outside 1 .. 16, a NaN or negative beta, a NaN
 * threshold, bg outside [-1, S), mode outside 0 .. 2, S > 4096, a window of sr_timeline_decide with a count < 1, more than 2^30
 * windows, a null argument; a process forked after the GPU runtime was initialised is refused as well.
 * Timer kinds (none is added): SR_T_CMVN the sum kernel; SR_T_SCORE_REF the decision and forward kernels; SR_T_ESTEP the traceback. */
int64_t sr_timeline_windows(int64_t n_frames, int64_t window, int64_t hop);
int sr_timeline_plan(int S, int min_dur, int64_t n_frames, int window, int hop, int32_t *out, int n_out);
int sr_timeline_decide(const double *sums, const int32_t *counts, const int64_t *win_off, int U, int S, int bg, double threshold, int mode,
                       double beta, int min_dur, int *label_out, double *path_score_out, int64_t *bad_windows_out);
int sr_timeline_batch(SRModelSet *set, SRBatch *features, int window, int hop, int bg, double threshold, int mode, double beta, int min_dur,
                      int flags, int64_t *win_off_out, int *label_out, double *sums_out, double *path_score_out, int64_t *bad_windows_out);
int sr_fullset_timeline_batch(SRFullSet *set, SRBatch *features, int window, int hop, double threshold, int mode, double beta, int min_dur,
                              int64_t *win_off_out, int *label_out, double *sums_out, double *path_score_out, int64_t *bad_windows_out);
int sr_timeline_pcm_batch(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int window, int hop, int bg, double threshold, int mode,
                          double beta, int min_dur, int flags, int64_t *win_off_out, int *label_out, double *sums_out, double *path_score_out,
                          int64_t *bad_windows_out);

/* ---- Who spoke when, nobody enrolled: BIC segments and agglomerative clustering on the device (csrc/diar.hip) ----
 * A feature batch of U recordings, [n_u][D] fp32, resident; 1 <= D <= 64.  All arithmetic below is float64, nothing is fused.
 *   base segments   L >= 1 frames each: n_seg = floor(n / L), or 1 if that is 0 and n > 0, or 0 if n = 0 (sr_diar_segments).  Segment i
 *                   covers frames [i L, (i + 1) L); the last reaches to n.
 *   statistics      of a segment or a cluster, diar_stat_len = 1 + D + D (D + 1) / 2 doubles: N (the frame count), s[D] = sum x,
 *                   Q[D (D + 1) / 2] = sum x x^T, the lower triangle by rows.  Every entry is summed in frame order, one product and one
 *                   add per frame.  A merge adds statistics element by element: stat_i = stat_i + stat_j.
 *   logdet          Sigma = (Q - s s^T / N) / N + ridge I, ridge >= 0; ld = 2 sum_r log L_rr of its lower Cholesky factor.  A pivot that
 *                   is not finite or not positive fails the cluster: every distance that involves it is +inf, it never merges, and the
 *                   initial clusters that failed are counted per recording (fail_out).
 *   delta-BIC       dBIC(a, b) = 1/2 [(N_a + N_b) ld_ab - N_a ld_a - N_b ld_b] - lambda 1/2 (D + D (D + 1) / 2) log(N_a + N_b), lambda > 0;
 *                   ld_ab is the logdet of the summed statistics.  Negative: one Gaussian explains both.
 *   change          mode 1 ("bic"): for each boundary b = 1 .. n_seg - 1 and half-width m >= 1 segments, c[b] = dBIC(the sum of segments
 *                   [max(0, b - m), b), the sum of segments [b, min(n_seg, b + m))), the sums taken in index order (+inf when a
 *                   factorisation fails).  b is kept iff c[b] > 0, c[b] >= c[b'] for every b' with |b - b'| < m, and no earlier b' in
 *                   that range has the same value.  The initial clusters are the runs of base segments between kept boundaries, their
 *                   statistics the sums of their segments in index order.  Mode 0 ("uniform"): every base segment is an initial cluster.
 *   agglomeration   per recording: alive flags, statistics, ld and a table of distances of which the entries i < j are used.  A step:
 *                   the live pair (i, j), i < j, of smallest distance, the first in row-major order among equals; stop unless
 *                   live > k_max (k_max > 0; 0: no cap), or live > k_min and d < threshold; stop also when that distance is +inf;
 *                   otherwise merge j into i: add the statistics, mark j dead, recompute ld_i and dist(i, k) for every live k.
 *                   The root of a cluster is its smallest member; labels number the final clusters by first appearance.
 *   matrix mode     the same loop on a symmetric dissimilarity [n][n], n <= 4096: linkage 0 average, (c_i d_ik + c_j d_jk) / (c_i + c_j)
 *                   over the cluster sizes c (two products, one add, one division); 1 complete (the larger); 2 single (the smaller).
 *                   The same argmin, tie order, log and labels.
 * sr_diar_segments: n_seg as above (0 for n <= 0 or L < 1).  Host only.
 * sr_diar_plan: what a call decides (csrc/diar_plan.cpp; host only) for recordings of lengths[U] frames under a bound of scratch_bytes
 *   (<= 0: the option diar_scratch_mib, default 1024).  Writes 16 fields (n_out >= 16): the factorisation's bucket width (D rounded up
 *   to 16 / 32 / 48 / 64), the doubles of a statistic, the entries of (s, Q) a lane of the statistics kernel owns, its lanes, the
 *   frames it stages at a time, its LDS bytes, the change kernel's LDS bytes, the number of groups, the built limits of D (64) and of a
 *   recording's initial clusters (4096), the waves (matrices) per workgroup of the pair / row kernels, the argmin kernel's workgroups per
 *   recording at most (its workgroups hold 256 lanes), the steps between two reads of the stop word, the bytes of all recordings, the
 *   bound, 0.  group_begin_out[groups + 1] (recordings [g, g + 1) run together) and rec_out[U][3] (base segments, the most initial
 *   clusters, bytes on the device) may be NULL.  Returns the number of groups, -1 on refusal.  A recording whose tables exceed the bound
 *   on its own is refused with the byte count and the remedy (a longer L); a group holds at most 65535 recordings.  The results do not
 *   depend on the bound, bit for bit.
 * sr_diar_stats_batch: the statistics of the base segments, brought home: seg_off_out[U + 1], stats_out[n_seg_total][diar_stat_len]
 *   (cap: the segments stats_out holds).  The direct test of that kernel.
 * sr_diar_bic_matrix: dBIC of every pair of n <= 4096 clusters from statistics in host memory: out[n][n] (symmetric, 0 on the diagonal),
 *   ld_out[n] (NaN for a cluster that failed; may be NULL), *fail_out the count of those (may be NULL).  The direct test of the
 *   factorisation.
 * sr_diar_cluster_batch: the whole chain.  cap: the entries the per-cluster outputs hold (the batch's base segments always suffice).
 *   init_cl_off_out[U + 1]: the initial clusters of the recordings; init_off_out[cap + U]: per recording n_init + 1 run boundaries in
 *   base-segment indices, recording u's at init_cl_off[u] + u; label_out[cap]: a label per initial cluster; merge_i_out, merge_j_out,
 *   merge_d_out[cap] (may be NULL): recording u's log in its first n_merges_out[u] entries from init_cl_off[u] (zeros behind);
 *   n_merges_out, n_clusters_out, fail_out[U] (may be NULL).  The merge log is a dendrogram: sr_diar_cut re-cuts it on the host.
 * sr_diar_cluster_pcm_batch: sr_mfcc_extract_batch (CMVN, nd orders of deltas) on resident PCM, then sr_diar_cluster_batch; the
 *   features stay on the device.  Frame counts: sr_mfcc_num_frames; the plan's refusals are made from them, before the feature stage runs.
 * sr_ahc_matrix: the matrix mode.  merge_*_out[n - 1], label_out[n].
 * sr_diar_cut: the labels a stop rule gives on a merge log (the steps it takes are a prefix of the log).  Returns the number of
 *   clusters, -1 on refusal; *n_merges_out the steps taken.  Host only.
 * The results are the same bits from run to run and do not depend on the recordings clustered in the same call (no atomics).
 * Refused, before the device is touched, with the remedy: D > 64; L < 1, m < 1, lambda <= 0, ridge < 0, a non-finite lambda or ridge, a
 * NaN threshold; k_min < 1, k_max in 1 .. k_min - 1 or negative; a change mode outside 0 .. 1; more than 4096 initial clusters (uniform
 * mode; bic mode refuses once the detector has counted them); a NaN, -inf or asymmetric matrix, linkage outside 0 .. 2; a null argument;
 * a process forked after the GPU runtime was initialised.
 * Timer kinds (none is added): SR_T_CMVN the statistics and gather kernels; SR_T_SCORE_REF the factorisations (logdet, pairs, change,
 * rows); SR_T_ESTEP the argmin and merge kernels. */
int64_t sr_diar_segments(int64_t n_frames, int64_t L);
int sr_diar_plan(int D, int L, int change, const int64_t *lengths, int U, int64_t scratch_bytes, int64_t *out, int n_out,
                 int32_t *group_begin_out, int64_t *rec_out);
int sr_diar_stats_batch(SRBatch *features, int L, int64_t cap, int64_t *seg_off_out, double *stats_out);
int sr_diar_bic_matrix(int D, int64_t n, const double *stats, double lambda, double ridge, double *out, double *ld_out, int64_t *fail_out);
int sr_diar_cluster_batch(SRBatch *features, int L, int change, int m, double lambda, double ridge, double threshold, int k_min, int k_max,
                          int64_t cap, int64_t *init_cl_off_out, int64_t *init_off_out, int32_t *merge_i_out, int32_t *merge_j_out,
                          double *merge_d_out, int32_t *label_out, int64_t *n_merges_out, int64_t *n_clusters_out, int64_t *fail_out);
int sr_diar_cluster_pcm_batch(SRMfcc *m, SRBatch *pcm, int nd, int L, int change, int half_width, double lambda, double ridge, double threshold,
                              int k_min, int k_max, int64_t cap, int64_t *init_cl_off_out, int64_t *init_off_out, int32_t *merge_i_out,
                              int32_t *merge_j_out, double *merge_d_out, int32_t *label_out, int64_t *n_merges_out, int64_t *n_clusters_out,
                              int64_t *fail_out);
int sr_ahc_matrix(int64_t n, const double *dist, int linkage, double threshold, int k_min, int k_max, int32_t *merge_i_out, int32_t *merge_j_out,
                  double *merge_d_out, int64_t *n_merges_out, int32_t *label_out, int64_t *n_clusters_out);
int64_t sr_diar_cut(int64_t n, const int32_t *merge_i, const int32_t *merge_j, const double *merge_d, int64_t n_merges, double threshold,
                    int k_min, int k_max, int32_t *label_out, int64_t *n_merges_out);

/* ---- Speaker embeddings from a neural network the caller brings: x-vector forward pass on the device (csrc/xvector.hip) ----
 * A network is an ordered list of layers that ends at the embedding layer: frame layers (kind 0, tdnn: a dilated 1-D convolution
 * over integer frame offsets), exactly one pooling layer (kind 1, stats_pool: mean and standard deviation over a segment's remaining
 * frames), then segment layers (kind 2, affine).  A tdnn or affine layer computes  y = scale * act(W x_ctx + b) + shift  per channel
 * (affine, activation, batch-norm: Kaldi's order; a batch-norm in front of the activation is folded into W and b by the caller, with
 * scale and shift left out).  Valid convolution only: over a segment of T input frames output frame u is
 * b + sum_j W_j x[u + o_j - o_1], u = 0 .. T - (o_m - o_1) - 1.
 * Descriptor table: 16 int32 per layer {kind, c_in, c_out, act (0 none, 1 relu), 1 when scale and shift are given, number of offsets
 * m, offsets[9], 0}; var_floor[n_layers] (read for the pooling layer); W[l]: float [c_out][m * c_in], offset-major; b, scale, shift[l]:
 * float [c_out] (scale[l] and shift[l] NULL together, or the arrays themselves NULL).  Entries of a pooling layer are ignored.
 * Arithmetic: weights are rounded once to bf16 (round to nearest even) by sr_xvector_create; features are fp32, rounded to bf16 by a
 * convert kernel; every layer accumulates in fp32 on the bf16 matrix cores in an order that depends on the layer alone (offsets
 * ascending, channels ascending inside an offset); the epilogue runs in fp32: z = acc + b, a = act(z), y = fma(scale, a, shift);
 * activations are stored as bf16 (round to nearest even), the last layer and a tapped layer as fp32.  The pooling reads the bf16
 * activations and sums x and x^2 in float64 in an order that depends on the segment's frame count alone (no atomics):
 * std = sqrt(max(sum x^2 / n - mean^2, var_floor)); it writes [mean | std] as fp32.  A segment's embedding is the same bits alone,
 * in any batch, at any position of a batch, under any "xvector_scratch_mib" and from run to run.
 * sr_xvector_create needs no device (the weights go there with the first forward pass and stay).  sr_xvector_info writes 12 fields:
 * layers, the pooling layer's index, input width, embedding width, context (frames consumed: a segment needs context + 1), the layer
 * kernel's tile rows, tile columns, K per stage, channel granule, LDS bytes, workgroup size, the device the weights live on (-1: none yet).
 * sr_xvector_plan: host only.  lengths[n_seg]: the segments' frames.  Writes 16 fields: tile rows, tile columns, K per stage, granule,
 * context, embedding width, chunks, LDS bytes, the pooling layer's index, the last layer that runs, the result's rows and columns, the
 * bytes of the two ping-ponged activation buffers, the largest chunk's bytes, the bound (scratch_bytes <= 0: the option
 * "xvector_scratch_mib", 1 .. 2^20, default 1024).  Optional outputs: width_pad_out[n_layers + 1] the stages' padded widths;
 * rows_out[(n_layers + 1) * n_seg] every segment's rows at every stage; chunk_begin_out[chunks + 1]; tile_count_out[n_layers * chunks];
 * tiles_out[3 * tiles_cap]: layer tile_layer's tile list of chunk tile_chunk as (segment within the chunk, first output row, rows).
 * A chunk is whole segments; a segment costs its two largest frame-level activations (they are ping-ponged) plus its rows of the
 * segment-level stages and of the result.  Returns the number of chunks.
 * sr_xvector_extract_batch: a resident feature batch; segs: NULL (one segment per utterance) or int32 [n_seg][3] (utterance, first
 * frame, frames).  tap: -1 for the embeddings, fp32 [n_seg][E]; a layer's index for that layer's output instead: fp32 [sum of rows]
 * [c_out] for a frame layer, [n_seg][2 C] for the pooling, [n_seg][c_out] for a segment layer.  tap_bf16 != 0: the tapped layer stores
 * bf16 as it does inside the network and the result is those values widened.  out_cap: floats `out` holds.  times_ms_out: NULL or
 * [n_layers + 1]: the device time of the convert kernels [0] and of every layer [1 + l] (the call's own events; no timer kind is added).
 * sr_xvector_extract: the same from host rows X[n_rows][dim] and offsets[n_utt + 1].
 * Refused, before the device is touched, with the remedy: widths outside 1 .. 4096; more than 9 offsets, an offset outside -16 .. 16,
 * offsets that do not ascend; consecutive layers that disagree; no stats_pool, more than one, or none followed by an affine layer; a
 * last layer whose act is not none; non-finite weights; non-finite host features; a feature width other than the first layer's; a
 * segment outside its utterance or shorter than context + 1 (names the segment and the frames needed); a segment whose activations
 * alone exceed the bound (names the bytes); a null argument; a process forked after the GPU runtime was initialised. */
typedef struct SRXvector SRXvector;
SRXvector *sr_xvector_create(int n_layers, const int32_t *desc, const double *var_floor, const float *const *W, const float *const *b,
                             const float *const *scale, const float *const *shift);
void sr_xvector_free(SRXvector *net);
int sr_xvector_info(SRXvector *net, int32_t *out, int n_out);
int sr_xvector_plan(int n_layers, const int32_t *desc, const double *var_floor, const int64_t *lengths, int64_t n_seg, int tap, int tap_bf16,
                    int64_t scratch_bytes, int64_t *out, int n_out, int32_t *width_pad_out, int64_t *rows_out, int64_t *chunk_begin_out,
                    int64_t *tile_count_out, int tile_layer, int64_t tile_chunk, int32_t *tiles_out, int64_t tiles_cap);
int sr_xvector_extract_batch(SRXvector *net, SRBatch *features, const int32_t *segs, int64_t n_seg, int tap, int tap_bf16, float *out,
                             int64_t out_cap, double *times_ms_out);
int sr_xvector_extract(SRXvector *net, const float *X, int64_t n_rows, int dim, const int64_t *offsets, int n_utt, const int32_t *segs,
                       int64_t n_seg, int tap, int tap_bf16, float *out, int64_t out_cap, double *times_ms_out);

#ifdef __cplusplus
}
#endif
#endif /* PYGMM_HIP_H */
