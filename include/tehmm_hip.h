/*
 * tehmm_hip.h -- C ABI of libtehmm_hip.so, the MI355X (gfx950) implementation of teHmm's hot path.
 *
 * The library is a drop-in for the seven Cython functions the reference's Python model API calls
 * (hmm.py:57 `from . import _hmm`, emission.py:19 `from ._emission import ...`) plus fused,
 * device-resident entry points for the three drivers built on them (BaseHMM.decode,
 * BaseHMM.score_samples and the Baum-Welch E-step of BaseHMM.fit).
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns 0 on success or a
 *     negative TEHMM_ERR_* code (tehmm_last_error() gives the message for the calling thread);
 *   - all floating point is IEEE fp64, arrays are C-contiguous, little-endian;
 *   - "host" pointers are ordinary process memory owned by the caller (like the NumPy buffers the
 *     Cython functions receive); the callee never keeps them after returning;
 *   - segRatios may be NULL ("None" in the reference);
 *   - handles are opaque, tied to the HIP device that was current when they were created, and are
 *     safe to use from one thread at a time.
 *
 * Citations are file:line in glennhickey/teHmm.
 */
#ifndef TEHMM_HIP_H
#define TEHMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEHMM_OK 0
#define TEHMM_ERR_ARG (-1)         /* bad argument (NULL, negative size, N out of range ...) */
#define TEHMM_ERR_HIP (-2)         /* HIP runtime error (no device, out of memory, launch failure) */
#define TEHMM_ERR_UNSUPPORTED (-3) /* shape outside what the kernels support (see tehmm_max_states) */

/* ---- library / device ---------------------------------------------------------------------- */
int tehmm_abi_version(void);                 /* 4; later additions (map decode, emission distribution) are detected by symbol */
const char *tehmm_last_error(void);          /* thread-local message of the last failing call */
int tehmm_device_count(int *count);          /* hipGetDeviceCount */
int tehmm_set_device(int device);            /* hipSetDevice; one process per GPU calls this once */
int tehmm_max_states(void);                  /* largest N of the fused / chunk-parallel paths and the device
                                                 E-step and M-step (128) */
int tehmm_max_states_any(void);              /* largest N any entry point accepts (1024): above 128 states a model
                                                 evaluates through the sequential kernels of tehmm_large.hip.h */

/* ---- array-level entry points: 1:1 replacements of the Cython module functions --------------
 * Caller owns every buffer (host memory); results are written in place exactly where the Cython
 * functions write them. */

/* _emission.fastAllLogProbs -> _fastAllLogProbsU8/U16/32 (_emission.pyx:20-144).
 * obs [T][K], logProbs [K][N][S], outProbs [T][N]; includes the leading-rows quirk (pyx:73-80). */
int tehmm_emission_u8(int64_t T, int K, int N, int S, const uint8_t *obs, const double *logProbs,
                      double normalize, const double *segRatios, double *outProbs);
int tehmm_emission_u16(int64_t T, int K, int N, int S, const uint16_t *obs, const double *logProbs,
                       double normalize, const double *segRatios, double *outProbs);
int tehmm_emission_i32(int64_t T, int K, int N, int S, const int32_t *obs, const double *logProbs,
                       double normalize, const double *segRatios, double *outProbs);

/* _hmm._forward (_hmm.pyx:120-158): fwdlattice [T][N] out. */
int tehmm_forward(int64_t T, int N, const double *log_startprob, const double *log_transmat,
                  const double *framelogprob, const double *segRatios, double *fwdlattice);

/* _hmm._backward (_hmm.pyx:160-198): bwdlattice [T][N] out. */
int tehmm_backward(int64_t T, int N, const double *log_startprob, const double *log_transmat,
                   const double *framelogprob, const double *segRatios, double *bwdlattice);

/* _hmm._viterbi (_hmm.pyx:201-259): state_sequence int64 [T] out, *logprob out. */
int tehmm_viterbi(int64_t T, int N, const double *log_startprob, const double *log_transmat,
                  const double *segRatios, const double *framelogprob, int64_t *state_sequence,
                  double *logprob);

/* _hmm._log_sum_lneta (_hmm.pyx:62-117): logsum_lneta [N][N] in/out (caller zero-fills it,
 * hmm.py:557). */
int tehmm_xi_logsum(int64_t T, int N, const double *fwdlattice, const double *log_transmat,
                    const double *bwdlattice, const double *framelogprob, double logprob,
                    const double *segRatios, double *logsum_lneta);

/* _emission.fastAccumulateStats -> _fastAccumulateStatsU8/U16/32 (_emission.pyx:146-234):
 * obsStats [K][N][S] += ... in place, in the reference's accumulation order. */
int tehmm_accumulate_obs_u8(int64_t T, int K, int N, int S, const uint8_t *obs, double *obsStats,
                            const double *posteriors, const double *segRatios);
int tehmm_accumulate_obs_u16(int64_t T, int K, int N, int S, const uint16_t *obs, double *obsStats,
                             const double *posteriors, const double *segRatios);
int tehmm_accumulate_obs_i32(int64_t T, int K, int N, int S, const int32_t *obs, double *obsStats,
                             const double *posteriors, const double *segRatios);

/* _emission.fastUpdateCounts -> _fastUpdateCountsU8/U16/32 (_emission.pyx:236-332), batched over the
 * labelled intervals of ONE table (the reference calls it once per overlap, emission.py:307-322):
 *   for i in 0..n_intervals-1, pos in [starts[i], ends[i]):      (table-relative coordinates)
 *     obsStats[track][states[i]][obs[pos][track]] += segRatios ? segRatios[pos] : 1.0
 * in that order (so ratio sums round as in the reference).  obs [T][K], obsStats [K][N][S] in place. */
int tehmm_update_counts_u8(int64_t T, int K, int N, int S, const uint8_t *obs, int n_intervals,
                           const int64_t *starts, const int64_t *ends, const int32_t *states,
                           const double *segRatios, double *obsStats);
int tehmm_update_counts_u16(int64_t T, int K, int N, int S, const uint16_t *obs, int n_intervals,
                            const int64_t *starts, const int64_t *ends, const int32_t *states,
                            const double *segRatios, double *obsStats);
int tehmm_update_counts_i32(int64_t T, int K, int N, int S, const int32_t *obs, int n_intervals,
                            const int64_t *starts, const int64_t *ends, const int32_t *states,
                            const double *segRatios, double *obsStats);

/* ---- fused, device-resident entry points ------------------------------------------------------
 * A model handle keeps the N x N log-transition matrix, start vector and emission tables on the
 * device; a batch handle keeps the observation columns (and segment ratios) of many independent
 * intervals (TrackTables) on the device, plus the result buffers.  One call then runs a whole
 * driver of the reference over every interval of the batch. */
typedef struct tehmm_model tehmm_model_t;
typedef struct tehmm_batch tehmm_batch_t;

/* Model state the reference keeps in MultitrackHmm._log_transmat / _log_startprob (hmm.py:625-666)
 * and emissionModel.logProbs [K][N][S] + normalizeFac (emission.py:44,58-60).
 * symbolsPerTrack (may be NULL) = emissionModel.numSymbolsPerTrack: lets the library pack the
 * table raggedly (symbols 0..symbolsPerTrack[k] of track k); with NULL all S columns are kept. */
/* N up to 1024 (K <= 128, S <= 256; larger: TEHMM_ERR_UNSUPPORTED before any device call).  Above 128 states the
 * handle keeps only the tables of the sequential large-state kernels: tehmm_eval_batch, the result calls and
 * tehmm_model_get_params take it, while the batch E-step, M-step and statistics calls return TEHMM_ERR_UNSUPPORTED. */
int tehmm_model_create(int N, int K, int S, const double *log_transmat, const double *log_startprob,
                       const double *logProbs, double normalize, const int32_t *symbolsPerTrack,
                       tehmm_model_t **out);
int tehmm_model_destroy(tehmm_model_t *model);

/* Observations of n_intervals TrackTables, concatenated: interval i is rows
 * offsets[i] .. offsets[i+1]-1 of obs [total][K] (uint8, IntegerTrackTable.data, track.py:555) and
 * of segRatios [total] (may be NULL).  obs_on_device != 0: obs/segRatios are device pointers on
 * the current device (the data stays where it is and is repacked by a kernel on the batch's own stream, after
 * the work queued on the default stream; a producer on any other stream must have finished). */
int tehmm_batch_create(int n_intervals, const int64_t *offsets, int K, const uint8_t *obs,
                       const double *segRatios, int obs_on_device, tehmm_batch_t **out);
/* The same from the other two observation types of the reference (IntegerTrackTable with uint16 / int32 data:
 * _fastAllLogProbsU16 / 32, _fastAccumulateStatsU16 / 32, _emission.pyx:82-144, 192-234), host arrays only.  The fused
 * kernels keep one byte per track and position: a symbol outside 0..255 returns TEHMM_ERR_UNSUPPORTED (such tables go
 * through the array-level entry points, which take all three types). */
int tehmm_batch_create_u16(int n_intervals, const int64_t *offsets, int K, const uint16_t *obs,
                           const double *segRatios, tehmm_batch_t **out);
int tehmm_batch_create_i32(int n_intervals, const int64_t *offsets, int K, const int32_t *obs,
                           const double *segRatios, tehmm_batch_t **out);
int tehmm_batch_destroy(tehmm_batch_t *batch);
int64_t tehmm_batch_total(const tehmm_batch_t *batch);
/* Forgets what earlier evaluations derived from the batch's observations for a model (the table-row index
 * records of the fused posterior passes): the next call pays for them again, as the first evaluation of a
 * fresh batch does.  bench.py calls it before every timed step -- teHmmEval evaluates a batch once. */
int tehmm_batch_reset_cache(tehmm_batch_t *batch);

/* Flags for tehmm_eval_batch. */
#define TEHMM_EVAL_VITERBI 1   /* BaseHMM.decode -> _decode_viterbi (basehmm.py:301-330, 361-396) */
#define TEHMM_EVAL_POSTERIOR 2 /* BaseHMM.score_samples (basehmm.py:238-273) */
#define TEHMM_EVAL_USE_RATIOS 4 /* the batch's segRatios apply the way the reference applies them:
                                   decode: transitions only (Q11); score_samples: never (Q12) */

/* Runs decode and/or score_samples over every interval.  Results stay on the device (fetch with
 * the tehmm_batch_get_* calls); viterbi_logprob / forward_logprob [n_intervals] are host arrays
 * (may be NULL). */
int tehmm_eval_batch(tehmm_model_t *model, tehmm_batch_t *batch, int flags,
                     double *viterbi_logprob, double *forward_logprob);

/* Copy results of the last tehmm_eval_batch to host memory: paths int64 [total] (the concatenated
 * state sequences), posteriors [total][N]; row range [row0,row1) of the concatenation. */
int tehmm_batch_get_paths(tehmm_batch_t *batch, int64_t row0, int64_t row1, int64_t *paths);
int tehmm_batch_get_posteriors(tehmm_batch_t *batch, int64_t row0, int64_t row1, double *post);
/* Pinned host memory for the destinations above (one DMA at link speed instead of the runtime's bounce buffers;
 * any other destination is staged in 32 MB pieces through two pinned buffers).  Freed blocks are cached in the
 * library -- pinning is the slow part -- up to 24 GB. */
int tehmm_host_alloc(size_t bytes, void **out);
int tehmm_host_free(void *ptr);
/* The library also keeps the DEVICE blocks of destroyed batches for the next batch (a fresh batch per call allocates the
 * same workspaces again; hipMalloc of memory the process has just returned can cost hundreds of milliseconds): up to
 * TEHMM_DEVICE_POOL_GB (environment, default 48, 0 = no caching).  tehmm_trim_pools returns every cached device and
 * pinned host block to the system (call it before handing the GPU to another allocator that needs the room). */
int tehmm_trim_pools(void);
/* Device pointers of the same buffers (valid until the batch is destroyed or re-evaluated). */
int tehmm_batch_device_ptrs(tehmm_batch_t *batch, void **paths_i64, void **posteriors_f64);

/* ---- output reductions: what teHmmEval writes per row (bin/teHmmEval.py:238-275) ----------------
 * Posterior column of --pd / --pdStates (:270-272): out[r - row0] = sum_j posteriors[r][j] * mask[j]
 * for rows [row0, row1) of the last evaluation's device-resident posteriors (8 instead of 8 N bytes
 * per row cross PCIe).  mask [N] and out are host arrays.  (The reference's off-by-one row, quirk
 * Q15, is the caller's: tehmm_amd/output.py.) */
int tehmm_batch_posterior_masksum(tehmm_batch_t *batch, const double *mask, int64_t row0, int64_t row1,
                                  double *out);
/* BaseHMM._decode_map (basehmm.py:332-359) over every interval, from the posteriors of the last
 * TEHMM_EVAL_POSTERIOR evaluation of this batch.  map_logprob [n_intervals] host (may be NULL) = the
 * reference's "logprob" (sum of the row maxima, quirk Q13).  mask [N] host or NULL; with a mask the
 * masked sums of the same rows are kept as well.  TEHMM_ERR_ARG when the batch holds no posterior result.
 * The state of a row is np.argmax of its posteriors: the lowest index among equal maxima, the first NaN of a
 * row that holds one.  The path has its own buffer (tehmm_batch_get_paths keeps the Viterbi path of a
 * VITERBI|POSTERIOR evaluation); the interval sums are taken in one fixed order, so two calls agree bit for
 * bit; the masked sums equal tehmm_batch_posterior_masksum's bit for bit.  The next tehmm_eval_batch drops
 * the result: the two getters then return TEHMM_ERR_ARG until tehmm_batch_map_decode has run again.
 * tehmm_batch_last_timing gains the entries "map_decode" and "map_logprob_sum". */
int tehmm_batch_map_decode(tehmm_batch_t *batch, const double *mask, double *map_logprob);
int tehmm_batch_get_map_paths(tehmm_batch_t *batch, int64_t row0, int64_t row1, int64_t *paths);
int tehmm_batch_get_map_masksum(tehmm_batch_t *batch, int64_t row0, int64_t row1, double *out);
/* array level, host buffers: states[t] = argmax_j post[t][j] (np.argmax rule), rowmax[t] (may be NULL);
 * any N from 1 to 1024 */
int tehmm_posterior_argmax(int64_t T, int N, const double *post, int64_t *states, double *rowmax);
/* MultitrackHmm.emissionDistribution + the --ed column (hmm.py:265-277, teHmmEval.py:273-275), from the packed
 * observations of the batch and the emission rows of the model; any N from 1 to 1024, no prior tehmm_eval_batch needed,
 * and no evaluation result of the batch (paths, posteriors, map result) is touched.
 *   tehmm_batch_get_emissions:    frame [row1 - row0][N] host = the rows fastAllLogProbs writes, bit for bit;
 *   tehmm_batch_emission_masksum: out [row1 - row0] host, out[r] = log(sum_j exp(frame[r][j]) * mask[j]) (mask [N] host),
 *                                 -inf where the sum is 0: 8 instead of 8 N bytes per row cross PCIe.
 * Rows [row0, row1) of the concatenation; the range may cross interval boundaries.  The leading-rows rule (quirk Q9: the
 * rows before the first emittable row are all zero) is applied per INTERVAL, as the reference calls the function once
 * per table, also when row0 lies behind an interval's leading rows.  use_ratios: multiply the rows by the batch's
 * segRatios (emissionDistribution hands the TrackTable itself to allLogProbs, so a segmented table does get them
 * there); TEHMM_ERR_ARG on a batch created without ratios.  Nothing is accumulated across rows: two calls agree bit for
 * bit.  tehmm_batch_last_timing gains "emission_column" / "emission_frame" (the device passes of the last such call).
 * (The one-row shift of the emission file, quirk Q15, is the caller's: tehmm_amd/output.py.) */
int tehmm_batch_emission_masksum(tehmm_model_t *model, tehmm_batch_t *batch, int use_ratios, const double *mask,
                                 int64_t row0, int64_t row1, double *out);
int tehmm_batch_get_emissions(tehmm_model_t *model, tehmm_batch_t *batch, int use_ratios, int64_t row0, int64_t row1,
                              double *frame);
/* BED coordinates of every row of a table (:243-266): segOffsets [n_rows] (NULL: unsegmented),
 * maskOffsets [n_mask] = TrackTable.getMaskRunningOffsets() (NULL: no mask); starts / ends [n_rows]. */
int tehmm_bed_coords(int64_t n_rows, int64_t table_start, int64_t table_end, const int64_t *segOffsets,
                     const int32_t *maskOffsets, int64_t n_mask, int64_t *starts, int64_t *ends);
/* Host-side writer of the per-row lines "chrom\tstart\tend\tX\n" (:266-275).  X = names[states[i]]
 * (names NULL: the integer) or, with values != NULL, values[i] as Python 2 prints a float64. */
int tehmm_write_bed(const char *path, int append, const char *chrom, int64_t n, const int64_t *starts,
                    const int64_t *ends, const int64_t *states, int n_names, const char *const *names,
                    const double *values);

/* Baum-Welch E-step over every interval of the batch (basehmm.py:504-523 with
 * MultitrackHmm._accumulate_sufficient_statistics, hmm.py:545-574): accumulates INTO the host
 * arrays start[N], trans[N][N], obsStats[K][N][S] (the caller initialises them, e.g. with
 * emission.initStats' fudge) and returns the summed forward log-likelihood.  use_ratios: apply
 * the batch's segRatios everywhere, as fit does for segmented TrackTables (emission rows scaled,
 * emission.py:195-196; lt[j][j] (r - 1) in the recurrences, _hmm.pyx:131-140; ratio-weighted posteriors in
 * the histograms, _emission.pyx:183-190; the diagonal term of _log_sum_lneta, _hmm.pyx:94-99).
 * N <= 128.  Below 64 states without ratios: the chunk-parallel fused passes with exact chains; with ratios,
 * and at 64..128 states: the item-parallel passes (warm-up + verified links); what those do not take (rows no
 * state can emit, links that never verify) runs on sequential kernels below 64 states and returns
 * TEHMM_ERR_UNSUPPORTED at 64 and above (the array-level entry points then serve the reference's own loop). */
int tehmm_estep_batch(tehmm_model_t *model, tehmm_batch_t *batch, int use_ratios, double *start,
                      double *trans, double *obsStats, double *logprob_sum);

/* ---- device-resident Baum-Welch ----------------------------------------------
 * The E-step's raw sufficient statistics stay on the device in ONE flat fp64 buffer
 * (tehmm_model_stats_size doubles: [logprob sum, sequence count, start, transition accumulators,
 * emission histograms]); buffers of several batches / ranks simply add (one all-reduce per EM
 * iteration over this buffer, basehmm.py:507-522 summed across shards), and tehmm_model_mstep turns the
 * sum into the next parameters without leaving the device (MultitrackHmm._do_mstep, hmm.py:576-616;
 * emission.maximize, emission.py:243-267; gaussian refit, emission.py:502-593, quirk Q19). */
int64_t tehmm_model_stats_size(const tehmm_model_t *model);
int tehmm_stats_alloc(const tehmm_model_t *model, double **dev_stats);   /* zero-filled device buffer */
int tehmm_stats_zero(const tehmm_model_t *model, double *dev_stats);
int tehmm_stats_free(double *dev_stats);
int tehmm_stats_head(const double *dev_stats, double *logprob_sum, double *n_sequences);
/* Copies the whole buffer device -> host (to_device = 0) or host -> device (to_device = 1): how a process group
 * whose backend cannot see device memory (gloo) sums the statistics of its ranks. */
int tehmm_stats_copy(const tehmm_model_t *model, double *dev_stats, double *host_buf, int to_device);
/* tehmm_estep_batch with the statistics ADDED into dev_stats (a device pointer: from tehmm_stats_alloc
 * or e.g. a torch tensor that RCCL will all-reduce). */
int tehmm_estep_batch_device(tehmm_model_t *model, tehmm_batch_t *batch, int use_ratios, double *dev_stats,
                             double *logprob_sum);
/* M-step: updates the model handle in place from the (summed) statistics.  update_*: the 's', 't', 'e'
 * of the reference's `params`; priors default to 1.0 there; fudge = emission model's fudge
 * (initStats + maximize); gaussian tracks: indices, the real value of every symbol
 * (gauss_values [n_gauss][S], CategoryMap.getMapBack) and the uniform mix (0.1); gauss_params
 * [n_gauss][N][2] (mu, sigma) out, may be NULL. */
int tehmm_model_mstep(tehmm_model_t *model, const double *dev_stats, int update_start, int update_trans,
                      int update_emission, double startprob_prior, double transmat_prior, double fudge,
                      int n_gauss, const int32_t *gauss_tracks, const double *gauss_values, double uniform_mix,
                      double *gauss_params);
/* Current parameters of the handle: log_transmat [N][N], log_startprob [N], logProbs [K][N][S] (only
 * the cells of real symbols are written); any pointer may be NULL. */
int tehmm_model_get_params(tehmm_model_t *model, double *log_transmat, double *log_startprob, double *logProbs);

/* ---- semi-supervised Baum-Welch: user constraints on the model handle (detected by symbol) --------
 * The reference re-applies its --forceTransProbs / --forceEmProbs / --forceStartProbs files after every M-step
 * (hmm.py:608-614).  Here the files become tables that live on the handle: uploaded once by this call and applied by
 * every later tehmm_model_mstep -- after its update kernels, before the derived layouts are rebuilt, in the
 * reference's order (transitions, emissions, start) and whatever the update_* flags say.
 *   trans_mask / trans_val [N][N], start_mask / start_val [N]: mask != 0 forces the cell to the probability in val;
 *     the other cells of the row (of the vector) are scaled to the mass that leaves, or zeroed when none is left
 *     (applyUserTrans, hmm.py:357-429; applyUserStarts, hmm.py:432-488);
 *   emis_mask / emis_val [K][N][S]: mask bit 0 forces the cell; bit 1, set on EVERY cell of a gaussian track, keeps
 *     the track's rows out of the rescale (a forced gaussian row is a whole row, filled by the caller from its
 *     (mu, sigma)).  Per (track, state) the unforced symbols are scaled, or -- when their mass is zero and the forced
 *     ones total less than 1 -- the leftover is added to them (applyUserEmissions, emission.py:347-438); then every
 *     real-symbol cell of every track goes through log(exp(x)) with zeros at -1e100, as the reference's closing myLog;
 *   trans_epsilons: the model's transMatEpsilons -- whenever a transition matrix with an exact zero is written (by the
 *     M-step's update or by the forced cells) machine epsilon is added to all its cells first (hmm.py:629-645: the
 *     setter drops the result of normalize(axis=1), so only that function's in-place `+= eps` takes effect).
 * Any pair may be NULL; all NULL with trans_epsilons = 0 clears the constraints.  Checked here, TEHMM_ERR_ARG: a mask
 * without its values, forced mass above 1, a (track, state) with every symbol forced to less than 1 in total.
 * TEHMM_ERR_UNSUPPORTED for N > 128.  What only the device can see (nothing learned left to scale under forced zeros:
 * the reference's assertion; a value that is not finite) makes the M-step return TEHMM_ERR_ARG, with the handle's
 * parameters those from before that call.  A constrained M-step adds no synchronisation and no upload to a plain
 * one, and copies one status word back.  None of this has been timed. */
int tehmm_model_set_constraints(tehmm_model_t *model, const uint8_t *trans_mask, const double *trans_val,
                                const uint8_t *start_mask, const double *start_val, const uint8_t *emis_mask,
                                const double *emis_val, int trans_epsilons);

/* ---- the step before the path: segment compression and mask compaction --------
 * TrackTable.segment = interpolateSegments + compressSegments (track.py:449-533, 594-620) for a uint8
 * table data [T][K] and ascending table-relative segOffsets [n_seg]: out [n_seg][K] holds the mode of
 * every categorical track over the segment; for gaussian tracks (is_gaussian[k] != 0) means [n_seg][K]
 * holds the mean of mapback[k][symbol] (mapback [K][256], CategoryMap.getMapBackTable) and out keeps
 * the segment's first symbol -- the caller maps the mean to a symbol (CategoryMap.getMap(update=True)
 * may create one, track.py:612-616). */
int tehmm_segment_table_u8(int64_t T, int K, const uint8_t *data, int64_t n_seg, const int64_t *segOffsets,
                           const uint8_t *is_gaussian, const double *mapback, uint8_t *out, double *means);
/* IntegerTrackTable.setMaskTable + getMaskRunningOffsets (track.py:622-662; _track.runSum,
 * _track.pyx:13-25): keep [T] = 1 where no mask track covers the position, run_full [T] = number of cut
 * positions before i, out_data [n_keep][K] / run_masked [n_keep] = the kept rows and their offsets. */
int tehmm_mask_table_u8(int64_t T, int K, const uint8_t *data, int KM, const uint8_t *maskdata, uint8_t *keep,
                        int32_t *run_full, uint8_t *out_data, int32_t *run_masked, int64_t *n_keep);

/* ---- the step before that: the segments themselves (bin/segmentTracks.py:200-277) ------
 * Cut rows of n_tables unsegmented uint8 tables, concatenated as tehmm_batch_create takes them: data
 * [total][K], table t = rows [table_offsets[t], table_offsets[t + 1]) (table_offsets[0] = 0, ascending, no
 * empty table).  Every table is a chain of its own, started at its first row; row i of a table opens a new
 * segment when (fixLen > 0) the running segment holds fixLen rows -- nothing else is looked at then -- or
 * (maxLen > 0) it holds maxLen rows, or row i differs from the segment's first row (comp_prev: from row
 * i - 1) in a track with cut[k] != 0 or in more than thresh tracks; tracks with ignore[k] != 0 never count.
 * Out: cuts = the table-relative offsets of every table's segments, ascending, table after table -- each
 * table's list starts with its 0, so n_cuts[t] >= 1 is its number of segments and segment n covers rows
 * [cuts[n], cuts[n + 1]) (the last one runs to the table's end); n_total = sum of n_cuts.  n_cuts and
 * n_total are always written; when n_total > cap, cuts is left untouched and the call still returns
 * TEHMM_OK (call again with a buffer of n_total).  stats_hist [K][K + 1] (NULL: not wanted): stats_hist[j][d]
 * = number of cuts made by the data rule at which track j differed and d tracks differed in all (the
 * reference's --stats: count[j] = sum_d hist[j][d], share[j] = sum_d hist[j][d] / d); cuts made by maxLen
 * or fixLen add nothing, as in the reference.
 * Checked before any device call: K <= 128 and total <= 2^31 - 1 (else TEHMM_ERR_UNSUPPORTED), thresh >= 0,
 * the table offsets, NULL pointers (TEHMM_ERR_ARG).  The output equals the reference's chain integer for integer on
 * every input; how the chain is cut into stripes and put together again: DESIGN.md section 5l. */
int tehmm_segment_offsets_u8(int n_tables, const int64_t *table_offsets, int K, const uint8_t *data,
                             const uint8_t *ignore, const uint8_t *cut, int thresh, int comp_prev, int64_t maxLen,
                             int64_t fixLen, int64_t cap, int64_t *cuts, int64_t *n_cuts, int64_t *n_total,
                             uint64_t *stats_hist);
/* Rows per stripe of the speculative pass. */
int64_t tehmm_segment_stripe_rows(void);
/* Of the calling thread's last tehmm_segment_offsets_u8: stripes of the speculative pass (0 where no chain was
 * needed: fixLen, or comp_prev without maxLen) and how many of them the link pass could not settle, so that the
 * exact sequential walk took them (marked stripes and the stripes walked again behind them). */
int tehmm_segment_last_counters(int64_t *stripes, int64_t *stripes_rewalked);
/* Device time of the passes of the calling thread's last tehmm_segment_offsets_u8, measured with HIP events
 * ("upload" and "download" include the host copies); returns the number of entries written. */
int tehmm_segment_last_timing(int max_entries, const char **names, double *milliseconds);
/* Host-side writer of the segment BED (segmentTracks.py:222-236): n lines "chrom\tstart\tend\tLABEL\n" with
 * LABEL = first_label + i in lower-case hexadecimal without a prefix (Python's hex(x)[2:]). */
int tehmm_write_segments_bed(const char *path, int append, const char *chrom, int64_t n, const int64_t *starts,
                             const int64_t *ends, int64_t first_label);

/* ---- the step after the path: judging a prediction against an annotation (bin/compareBedStates.py, ------
 * bin/fitStateNames.py).  An interval list is n rows (chrom id, start, end, label), host
 * arrays, uploaded by the call; chrom ids and labels are small integers the caller assigns (tehmm_amd/compare.py:
 * by first appearance, ONE label table for both lists of a comparison), coordinates are full int64 (a list's total
 * length must fit int64 too).  A list is valid when start < end, chrom ids never decrease, inside a chrom
 * start[i] >= end[i - 1], and every label lies in [0, L); two lists are comparable when they cover the same bases
 * (the reference's checkExactOverlap, which reads bed1 twice and so never looks at bed2's self-overlaps: both lists
 * are checked here).  Checked before any device call, by every entry point below: NULL pointers, n >= 1, L >= 1
 * (TEHMM_ERR_ARG); n <= 2^31 - 1 and L <= 2048 (TEHMM_ERR_UNSUPPORTED).
 *
 * tehmm_intervals_check: *which = 0 when both lists are valid and comparable, else 1 or 2 = the offending list and
 * *where = the interval's index; the call returns TEHMM_OK either way (tehmm_last_error then holds a sentence).
 * Order: validity of list 1, of list 2 (lowest index each), then the cover: the lowest interval of list 1 that starts
 * (ends) a region -- no predecessor (successor) abuts it -- where list 2 starts (ends) none, then the same for list 2. */
int tehmm_intervals_check(int64_t n1, const int32_t *chrom1, const int64_t *start1, const int64_t *end1,
                          const int32_t *label1, int64_t n2, const int32_t *chrom2, const int64_t *start2,
                          const int64_t *end2, const int32_t *label2, int L, int *which, int64_t *where);
/* compareBaseLevel (compareBedStates.py:176-221) in one number per pair of labels: conf [L][L] host, conf[a][b] =
 * bases labelled a in list 1 and b in list 2.  The reference's stats[s] = [FN, FP, TP] are row sum minus diagonal,
 * column sum minus diagonal and diagonal; its confusion dict holds the non-zero cells as [name b][name a].
 * first [L][L] host (NULL: not wanted): for every non-zero cell, (index in list 1 << 32 | index in list 2) of the two
 * intervals whose overlap is the first of that cell along the lists -- where the reference's walk inserts the pair
 * into its dicts, which is the order its later tie-breaks go by; -1 (all ones) in the other cells.
 * Runs the check above first: TEHMM_ERR_ARG, with the offender named in tehmm_last_error, on lists that fail it. */
int tehmm_compare_base(int64_t n1, const int32_t *chrom1, const int64_t *start1, const int64_t *end1,
                       const int32_t *label1, int64_t n2, const int32_t *chrom2, const int64_t *start2,
                       const int64_t *end2, const int32_t *label2, int L, int64_t *conf, int64_t *first);
/* One side of compareIntervalsOneSided (compareBedStates.py:223-313).  For every true interval t, over the preds
 * that overlap it, in list order: frac = (double)overlap / (double)(use_pred_len ? length of the pred : length of t);
 * where the labels are equal best = max(best, frac) and total += frac (both from 0.0, IEEE fp64, this order); where
 * frac >= threshold conf[label(pred)][label(t)] += 1.  t is a hit when (allow_multiple ? total : best) >= threshold.
 * Out, by the label of t: n_hit / len_hit / n_miss / len_miss [L] (lengths in bases) and conf [L][L], all host;
 * first [L][L] (NULL: not wanted) as in tehmm_compare_base, with (index of t << 32 | index of the pred).
 * Same check and error as tehmm_compare_base. */
int tehmm_compare_intervals(int64_t n_true, const int32_t *chrom_t, const int64_t *start_t, const int64_t *end_t,
                            const int32_t *label_t, int64_t n_pred, const int32_t *chrom_p, const int64_t *start_p,
                            const int64_t *end_p, const int32_t *label_p, int L, double threshold, int use_pred_len,
                            int allow_multiple, int64_t *n_hit, int64_t *len_hit, int64_t *n_miss, int64_t *len_miss,
                            int64_t *conf, int64_t *first);
/* The merge of writeFittedBed (fitStateNames.py:241-268): labels go through lut [L] first (NULL: as they are; the
 * values of lut are only compared, any int32 will do), then neighbours of equal chrom and mapped label with
 * start[i] == end[i - 1] become one interval.  Only the labels are checked (TEHMM_ERR_ARG outside [0, L)); the list
 * need not be valid.  On TEHMM_OK *n_out is written whatever cap is; when *n_out > cap the four outputs are left
 * untouched and the call still returns TEHMM_OK (call again with buffers of *n_out).  On an error nothing is written. */
int tehmm_merge_runs(int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, const int32_t *label,
                     int L, const int32_t *lut, int64_t cap, int32_t *out_chrom, int64_t *out_start, int64_t *out_end,
                     int32_t *out_label, int64_t *n_out);
/* Device time of the passes of the calling thread's last call of the four above, as tehmm_segment_last_timing. */
int tehmm_compare_last_timing(int max_entries, const char **names, double *milliseconds);
/* The largest L whose matrices are accumulated in LDS, one copy per workgroup flushed once; above it every add is a
 * 64-bit atomic on the global matrix. */
int tehmm_compare_lds_labels(void);
/* Intervals per workgroup of the run merge's count and scatter passes. */
int64_t tehmm_compare_block_items(void);

/* ---- Target site duplications (bin/tsdFinder.py on kmer.py) and the clean-up of bin/removeBedOverlaps.py ------------
 * tehmm_tsd_find: exact forward matches between the bases left and right of every element, as intervalTsds
 * (tsdFinder.py:242-298) finds them.  Sequences: n_seq records in one byte buffer, record q = bases[seq_offsets[q],
 * seq_offsets[q + 1]), upper or lower case.  Elements: seq_index / start / end [n], all host, in output order.
 * Options as the tool's: min_len (--min, the k-mer length), max_len (--max), left, right, overlap, all (0: the nearest
 * match of every element only) and max_score (--maxScore; -1: no filter; below -1 keeps nothing).
 * Out: counts [n] = matches of every element; the matches of all elements in element order, within an element in the
 * reference's list order, as six columns of *n_out rows: left start / end, d1 = |start - left end|, right start /
 * end, d2 = |end - right start| (coordinates inside the element's sequence).  On TEHMM_OK *n_out is the number of
 * matches whatever cap is, and the first min(*n_out, cap) rows of the columns are written (cap 0: the columns may be
 * NULL; call again with cap >= *n_out).  On an error *n_out is 0.
 * Checked before any device call: TEHMM_ERR_ARG for a NULL pointer, n_seq < 1, n < 1, cap < 0, min_len < 1,
 * min_len > max_len, min_len > 21 (hashDNA asserts there), decreasing seq_offsets, and the first element with a
 * seq_index outside [0, n_seq), start < 0 or start > end; TEHMM_ERR_UNSUPPORTED for n > 2^31 - 1 and for a search
 * window above tehmm_tsd_window() = 64 bases (left + overlap - 1 or right + overlap - 1).  Checked on the device:
 * TEHMM_ERR_ARG naming the lowest element with a base other than ACGTNacgtn inside a window that is searched (the
 * reference asserts there); bases outside every searched window are never read. */
int tehmm_tsd_find(int n_seq, const uint8_t *bases, const int64_t *seq_offsets, int64_t n, const int32_t *seq_index,
                   const int64_t *start, const int64_t *end, int min_len, int max_len, int left, int right, int overlap,
                   int max_score, int all, int32_t *counts, int64_t cap, int64_t *left_start, int64_t *left_end,
                   int64_t *d1, int64_t *right_start, int64_t *right_end, int64_t *d2, int64_t *n_out);
/* removeBedOverlaps.py:76-95 on a list sorted by (chrom_id, start): start = max(start, end of the last kept interval
 * of the chromosome), kept iff end > start.  Out: out_index (position in the list) and out_start (the new start) of
 * the kept intervals, in list order; cap / *n_out as in tehmm_tsd_find.  TEHMM_ERR_ARG for NULL lists, n < 1,
 * cap < 0 and, from the device, naming the first interval whose chrom_id or (inside a chrom_id) start is below its
 * predecessor's; TEHMM_ERR_UNSUPPORTED for n > 2^31 - 1. */
int tehmm_remove_overlaps(int64_t n, const int32_t *chrom_id, const int64_t *start, const int64_t *end, int64_t cap,
                          int64_t *out_index, int64_t *out_start, int64_t *n_out);
/* Device time of the passes of the calling thread's last call of the two above, as tehmm_segment_last_timing. */
int tehmm_tsd_last_timing(int max_entries, const char **names, double *milliseconds);
/* The longest search window tehmm_tsd_find serves, in bases. */
int tehmm_tsd_window(void);

/* ---- Mask intervals outside the HMM (cutOutMaskIntervals, bin/interpolateMaskedRegions.py) -------------------------
 * Interval lists are host columns (int32 chrom id, int64 start, int64 end), uploaded by the call.  The caller numbers
 * the chroms in the byte-wise order of their names, so that id order is the order of sortBed ("chr10" < "chr2").
 * A list is SORTED when chrom ids never decrease and, inside a chrom, starts never decrease; DISJOINT when
 * additionally start[i] >= end[i - 1] inside a chrom.
 * Every entry point checks before any device call: TEHMM_ERR_ARG for NULL pointers, n < 1, cap < 0;
 * TEHMM_ERR_UNSUPPORTED for n > 2^31 - 1.  Checked on the device, TEHMM_ERR_ARG with the lowest offending index in
 * tehmm_last_error: start < end for every interval, and the stated order of each list.
 * cap / *n_out as in tehmm_tsd_find: on TEHMM_OK *n_out is the number of rows whatever cap is and the first
 * min(*n_out, cap) rows are written (cap 0: the columns may be NULL); on an error *n_out is 0.
 * Additions to ABI version 4: detect them by symbol.
 *
 * tehmm_intervals_merge: the list is sorted.  A run goes on while start <= the largest end of the run so far
 * (overlapping AND abutting intervals merge, as mergeBed does by default); the run's interval is written iff
 * min_len <= end - start <= max_len (filterBedLengths folded in; 0 and INT64_MAX: no filter). */
int tehmm_intervals_merge(int64_t n, const int32_t *chrom_id, const int64_t *start, const int64_t *end, int64_t min_len,
                          int64_t max_len, int64_t cap, int32_t *out_chrom, int64_t *out_start, int64_t *out_end,
                          int64_t *n_out);
/* A: any intervals in any order, each treated on its own.  B: sorted and disjoint (abutting b are served).
 * subtract: for every a, in A's order, the maximal parts of a that no b covers, left to right.
 * intersect: for every a, in A's order, the part a shares with every b that overlaps it, in B's order.
 * out_src: the index of a.  The cost of the emit pass is bounded by the number of rows written, not by how many b
 * one a spans: every row is one lane that finds its a in the scanned counts and its piece from the two b beside it. */
int tehmm_intervals_subtract(int64_t nA, const int32_t *chromA, const int64_t *startA, const int64_t *endA, int64_t nB,
                             const int32_t *chromB, const int64_t *startB, const int64_t *endB, int64_t cap,
                             int64_t *out_src, int64_t *out_start, int64_t *out_end, int64_t *n_out);
int tehmm_intervals_intersect(int64_t nA, const int32_t *chromA, const int64_t *startA, const int64_t *endA, int64_t nB,
                              const int32_t *chromB, const int64_t *startB, const int64_t *endB, int64_t cap,
                              int64_t *out_src, int64_t *out_start, int64_t *out_end, int64_t *n_out);
/* The flank loop of interpolateMaskedRegions.py:117-162.  M: the merged masks, sorted and disjoint.  I: the
 * prediction, sorted, intervals of equal (chrom, start) by ascending end (the order of the reference's tuple sort);
 * labels in [0, L) (else TEHMM_ERR_ARG, from the device), L >= 1 (TEHMM_ERR_ARG), L <= 2048 (TEHMM_ERR_UNSUPPORTED).
 * two_sided / one_sided: uint8 [L] flags; two_sided NULL = every label, one_sided NULL = none.
 * out_label [nM]: -2 for a mask longer than max_len (not filled), -1 for the default, else a label.  For a mask,
 * p = the first interval whose (chrom, start, end) is not below the mask's.  The right candidate is I[p], the left
 * I[p - 1] (none when p = 0).  When no interval is at or above the mask there is NO right candidate and the left
 * candidate is I[nI - 2] (none when nI = 1): the reference's pointer has stopped on the last index.  A candidate gives
 * its label when it shares the chrom and abuts (left: end == mask start; right: start == mask end); one that shares
 * the chrom and overlaps the mask without abutting is the reference's assertion: TEHMM_ERR_ARG naming the lowest such
 * mask.  The label: only_default -> default; left == right -> left if flagged in two_sided, else default; left
 * flagged in one_sided -> left; right flagged in one_sided -> right; else default. */
int tehmm_mask_fill(int64_t nM, const int32_t *chromM, const int64_t *startM, const int64_t *endM, int64_t nI,
                    const int32_t *chromI, const int64_t *startI, const int64_t *endI, const int32_t *labelI, int L,
                    const uint8_t *two_sided, const uint8_t *one_sided, int only_default, int64_t max_len,
                    int32_t *out_label);
/* Device time of the passes of the calling thread's last call of the four above, as tehmm_segment_last_timing. */
int tehmm_masking_last_timing(int max_entries, const char **names, double *milliseconds);

/* ---- Track loading (trackIO.readBedData / readFastaData) ---------------------------------------------------------
 * Paints K tracks into data [T, K] (host, row-major, out).  T is the row space of one call: the concatenation of all
 * tables, records already clipped to their table and shifted into it.  fill [K]: the value of a row nothing covers.
 * kind [K]: 0 = a track of records, 1 = a track of sequence bytes.
 * Records of track k are rec_offsets[k] .. rec_offsets[k + 1] of rec_start / rec_end / rec_sym0 / rec_sym, sorted by
 * rec_start inside the track.  Row p takes its value from the LAST record i of the track with rec_start[i] <= p <
 * rec_end[i]: rec_sym0[i] when p == rec_start[i], else rec_sym[i] -- what painting the records in order leaves behind.
 * Sequence tracks own T bytes each of seq_bytes (seq_offsets [K + 1]: 0 bytes for a record track), a byte of 0 standing
 * for "no base"; row p is seq_lut[q][byte] for the q-th sequence track of the call (seq_lut [number of them][256]).
 * Checked before any device call: TEHMM_ERR_ARG for NULL pointers, T < 0, K < 1, K > 128, a kind other than 0 / 1,
 * offsets that do not start at 0 or decrease, a sequence track with records or without its T bytes;
 * TEHMM_ERR_UNSUPPORTED above 2^31 - 1 records.  Checked on the device: TEHMM_ERR_ARG naming the lowest record index
 * whose start lies before its predecessor's in the track or that fails 0 <= start < end <= T.  The cost of a row does not
 * depend on how many records cover it or on their lengths (block maxima of rec_end, fan-out 64). */
int tehmm_load_tracks_u8(int64_t T, int K, const uint8_t *fill, const uint8_t *kind, const int64_t *rec_offsets,
                         const int64_t *rec_start, const int64_t *rec_end, const uint8_t *rec_sym0,
                         const uint8_t *rec_sym, const int64_t *seq_offsets, const uint8_t *seq_bytes,
                         const uint8_t *seq_lut, uint8_t *data);
/* Device time of the passes of the calling thread's last tehmm_load_tracks_u8, tehmm_track_rows_won or
 * tehmm_load_tracks_f32, as tehmm_segment_last_timing. */
int tehmm_trackio_last_timing(int max_entries, const char **names, double *milliseconds);
/* Rows of a tile of the paint kernel (tests cross it). */
int64_t tehmm_trackio_tile_rows(void);

/* Track scaling (bin/setTrackScaling.py): what the per-base float array of a numeric track holds, from its record
 * list.  Record tracks only, lists as in tehmm_load_tracks_u8 (row p belongs to the LAST record i of its track with
 * rec_start[i] <= p < rec_end[i]); there is no first-row value: the tool never takes the delta branch.
 * tehmm_track_rows_won: won[i] (int64 [rec_offsets[K]]) = rows record i wins, uncovered[k] (int64 [K]) = rows of track
 * k that no record covers; the won of a track and its uncovered add up to T.
 * tehmm_load_tracks_f32: out [K][T] (track after track), out[k][p] = rec_val[winner of p] or fill[k].
 * Both make the checks of tehmm_load_tracks_u8 on T, K and the record lists, before and on the device, with its error
 * codes and its message about the lowest offending record.  Additions to ABI version 4: detect them by symbol. */
int tehmm_track_rows_won(int64_t T, int K, const int64_t *rec_offsets, const int64_t *rec_start,
                         const int64_t *rec_end, int64_t *won, int64_t *uncovered);
int tehmm_load_tracks_f32(int64_t T, int K, const float *fill, const int64_t *rec_offsets, const int64_t *rec_start,
                          const int64_t *rec_end, const float *rec_val, float *out);

/* ---- the per-row BED text of teHmmEval, formatted on the device (bin/teHmmEval.py:238-275) -----------
 * Writes, for every table of a list, its optional header line (verbatim; headers or headers[t] NULL: none) and one line
 * "chrom\tstart\tend\tX\n" per row, byte for byte what tehmm_bed_coords + tehmm_write_bed produce table by table.
 * Table t owns rows row_offsets[t] .. row_offsets[t + 1] of the column (row_offsets [n_tables + 1], from 0, a table may
 * be empty); segOffsets[t] [its rows] (NULL array or NULL entry: unsegmented), maskOffsets[t] [n_mask[t]] (NULL: none).
 * kind: TEHMM_BED_NAMES X = names[states[r]] (0 to 1024 names of any length; a state outside them is TEHMM_ERR_ARG and
 * the file is not touched), TEHMM_BED_INT X = states[r], TEHMM_BED_VALUE X = values[r] as tehmm_write_bed prints a
 * float64.  shift: row i of a table carries the column entry of its row i - 1 and row 0 that of its last row (quirk Q15).
 * The device formats every value whose rounding it can certify; the others (exact ties of the 12th digit and values
 * within 2^-40 of one, subnormals, magnitudes beyond 1e-289 .. 1e281, NaN with the sign bit) get the host's snprintf.
 * The work runs in stripes of stripe_rows items (rows and table headers; 0: 4 Mi), the copy-back of a stripe under the
 * fwrite of the one before, through two pinned blocks of the tehmm_host_alloc pool. */
#define TEHMM_BED_NAMES 0
#define TEHMM_BED_INT 1
#define TEHMM_BED_VALUE 2
int tehmm_bed_text_write(const char *path, int append, int n_tables, const char *const *chroms, const int64_t *table_start,
                         const int64_t *table_end, const int64_t *row_offsets, const int64_t *const *segOffsets,
                         const int32_t *const *maskOffsets, const int64_t *n_mask, const char *const *headers, int kind,
                         const int64_t *states, const double *values, int n_names, const char *const *names, int shift,
                         int64_t stripe_rows);
/* The same for tables that are the intervals interval0 .. interval0 + n_tables of a batch, the column taken from the
 * device: the Viterbi path of the last evaluation, the maximum-posterior path of the last tehmm_batch_map_decode
 * (names NULL: the integer state), the masked posterior sum (the column of tehmm_batch_posterior_masksum) or the masked
 * emission column (that of tehmm_batch_emission_masksum; model and use_ratios as there).  The two value columns are
 * computed inside the call and written with the one-row shift; no per-row column reaches the host.  TEHMM_ERR_ARG when
 * the batch does not hold the evaluation a source needs. */
#define TEHMM_BED_SRC_VITERBI 0
#define TEHMM_BED_SRC_MAP 1
#define TEHMM_BED_SRC_POSTERIOR 2
#define TEHMM_BED_SRC_EMISSION 3
int tehmm_batch_bed_text_write(tehmm_model_t *model, tehmm_batch_t *batch, int source, const double *mask, int use_ratios,
                               int interval0, int n_tables, const char *const *chroms, const int64_t *table_start,
                               const int64_t *table_end, const int64_t *const *segOffsets,
                               const int32_t *const *maskOffsets, const int64_t *n_mask, const char *const *headers,
                               int n_names, const char *const *names, const char *path, int append, int64_t stripe_rows);
/* Of the calling thread's last call of the two above: rows and bytes written, rows the host formatted; and the device
 * passes summed over the stripes ("measure", "scan", "patch", "emit"; "host": the null stream's idle time between
 * stripes), then the host's "copy_wait", "fwrite" and "wall", as tehmm_segment_last_timing. */
int tehmm_bed_text_last_counters(int64_t *rows, int64_t *bytes, int64_t *host_rows);
int tehmm_bed_text_last_timing(int max_entries, const char **names, double *milliseconds);
/* The value formatter of the two calls, run on the CPU (the same code the device runs; no GPU needed): text [24] gets
 * the characters of x, *certified = 1 when the device path certified its rounding, 0 when the text is the host's. */
int tehmm_bed_text_format_value(double x, char *text, int *certified);

/* ---- CYK decode of the grammar model (cfg.py:219-304, _cfg.pyx:16-89) ---------------------------------
 * Decodes a batch of intervals; all arrays are host pointers.  Interval t owns rows offsets[t] .. offsets[t + 1]
 * (offsets [n + 1], from 0, every interval at least one row) of emLogProbs [total][M] (the rows of allLogProbs), of
 * alignment [total] (NULL: no alignment track) and of trace.  is_nest [M] marks the pair states; logProbs1 [M][M][M]
 * and logProbs2 [M][M] are the reference's tables (every entry above -inf is a production, -1e100 included),
 * logPriors [M][2] is indexed [state][match], log_start [M].
 * Results: scores[t] = max over x of log_start[x] + dp[0][L-1][x], top[t] its first arg-max, trace [total] the state of
 * every row as float64 (the reference's array).  Scores, states and every dp cell equal the reference's bit for bit:
 * the additions run in its order, ties go to the candidate its scan meets first.
 * TEHMM_ERR_UNSUPPORTED before any allocation for M > 64 and for intervals whose workspace does not fit the device
 * (the message names the largest L that fits); TEHMM_ERR_ARG, after the results were copied, when a derivation reaches
 * a cell that no production fills (the reference's assertion).  Additions to ABI version 4: detect them by symbol. */
int tehmm_cyk_decode(int n_intervals, const int64_t *offsets, int M, const double *emLogProbs, const uint16_t *alignment,
                     int defAlignmentSymbol, const uint8_t *is_nest, const double *logProbs1, const double *logProbs2,
                     const double *logPriors, const double *log_start, double *scores, int64_t *top, double *trace);
/* Test accessor: the full table dp [L][L][M] of one interval, -inf below the diagonal as the reference leaves it. */
int tehmm_cyk_get_dp(int64_t L, int M, const double *emLogProbs, const uint16_t *alignment, int defAlignmentSymbol,
                     const uint8_t *is_nest, const double *logProbs1, const double *logProbs2, const double *logPriors,
                     const double *log_start, double *dp);
/* Device time of the passes of the calling thread's last call of the two above ("upload", "init", "fill",
 * "traceback", "copy_back"), then the host's "wall", as tehmm_segment_last_timing. */
int tehmm_cyk_last_timing(int max_entries, const char **names, double *milliseconds);
/* Bytes of device memory a decode of intervals of these lengths takes (no device call). */
int64_t tehmm_cyk_workspace_bytes(int n_intervals, const int64_t *lengths, int M);

/* ---- BED text parsed on the device (trackIO.bedRead and what BedFile builds from it) -------------------
 * tehmm_bed_parse_open takes the bytes of one file (host memory; a tehmm_host_alloc block makes the upload one DMA) and
 * parses them by bedRead's rule: lines end at "\n", "\r\n" or a lone "\r", a last line without a terminator counts, a
 * line whose first byte is '#' or that has fewer than three tab-separated fields is dropped.  The handle keeps the text
 * and the tables on the device until tehmm_bed_parse_close.  All results are in file order over the KEPT records.
 * TEHMM_ERR_UNSUPPORTED (nothing parsed; the caller's host route serves the file) when text plus columns exceed the
 * workspace budget -- seven eighths of the free device memory, pooled blocks counted as free, or
 * TEHMM_BED_PARSE_MAX_WORKSPACE bytes if that is less -- or when a record has 2^31 bytes or more.  A file with a byte
 * >= 0x80 is not parsed either: tehmm_bed_parse_counts reports high_bytes > 0 and the getters return TEHMM_ERR_ARG.
 * Additions to ABI version 4: detect them by symbol. */
typedef struct tehmm_bedparse tehmm_bedparse_t;
int tehmm_bed_parse_open(const void *text, int64_t n_bytes, tehmm_bedparse_t **out);
int tehmm_bed_parse_close(tehmm_bedparse_t *h);
int tehmm_bed_parse_counts(tehmm_bedparse_t *h, int64_t *lines, int64_t *records, int64_t *high_bytes);
/* line_start / line_len [records]: the record's bytes without its terminator; n_fields [records]; field_off / field_len
 * [records][6]: columns 0..5, offsets from the record's first byte, length -1 where the record has no such column. */
int tehmm_bed_parse_get_table(tehmm_bedparse_t *h, int64_t *line_start, int64_t *line_len, int32_t *n_fields,
                              int32_t *field_off, int32_t *field_len);
/* Column col (0..5) as numbers: kind 0 integers into ivalue, kind 1 floats into fvalue; status [records]: 0 certified
 * (the value equals Python's int() / float() of the field), 1 left to the host's int() / float(), 2 no such column.
 * Certified: integers [+-]?[0-9]{1,18}; floats [+-]? digits with at most one '.' and an optional [eE][+-]?digits, at
 * most 15 significant digits (first non-zero digit to the last digit) and |exponent - fraction digits| <= 22, or a
 * mantissa of zeros. */
int tehmm_bed_parse_get_numbers(tehmm_bedparse_t *h, int col, int kind, int64_t *ivalue, double *fvalue, uint8_t *status);
/* Column col (0..5) as codes: codes [records] numbers the distinct byte strings in order of first appearance (-1: no
 * such column), first_records [records] gets, for each of the *n_distinct values, the record it first appears in.
 * *n_missing / *n_empty count records without the column / with an empty value.  Values are found through a 64-bit hash
 * (TEHMM_BED_PARSE_HASH_BITS in the environment at open truncates it: tests) and every record is then compared byte
 * for byte with its value's first record; on any difference *fell_back = 1 and codes are not written. */
int tehmm_bed_parse_get_codes(tehmm_bedparse_t *h, int col, int64_t *codes, int64_t *first_records, int64_t *n_distinct,
                              int64_t *n_missing, int64_t *n_empty, int *fell_back);
/* The number routines of the kernels run on the CPU (the same code; no GPU needed): kind and *status as above. */
int tehmm_bed_parse_number(const char *text, int64_t len, int kind, int64_t *ivalue, double *fvalue, int *status);
/* Bytes of text one workgroup classifies (tests place line ends across this boundary). */
int64_t tehmm_bed_parse_tile_bytes(void);
/* Since the calling thread's last open: lines, kept records, integer and float fields left to the host, code columns
 * that fell back; and the device passes ("upload", "classify", "scan_tiles", "lines", "keep", "scan_lines", "fields",
 * then "ints" / "floats" / "hash", "verify", "codes" per getter), as tehmm_segment_last_timing. */
int tehmm_bed_parse_last_counters(int64_t *lines, int64_t *records, int64_t *host_ints, int64_t *host_floats,
                                  int64_t *code_fallbacks);
int tehmm_bed_parse_last_timing(int max_entries, const char **names, double *milliseconds);

/* Forward log-likelihood of every interval from the last tehmm_estep_batch or posterior evaluation
 * (the per-sequence `lpr` of basehmm.py:513, which MultitrackHmm's best-iteration bookkeeping,
 * hmm.py:690-711, consumes sequence by sequence); out [n_intervals] host. */
int tehmm_batch_get_interval_logprobs(tehmm_batch_t *batch, double *out);

/* Per-kernel device time of the last fused call on this batch, measured with HIP events on the
 * streams the kernels ran on.  names[i] is a static string; returns the number of entries
 * written (<= max_entries). */
int tehmm_batch_last_timing(tehmm_batch_t *batch, int max_entries, const char **names,
                            double *milliseconds);

/* Diagnostic builds only (-DTEHMM_STAMPS): per-wave cycle stamps of the last cooperative kernel,
 * [workgroup][wave][4] counters.  The product library returns TEHMM_ERR_UNSUPPORTED. */
int tehmm_debug_read_stamps(unsigned long long *out, int n);
/* Test-only: waits for the batch's streams and copies the index records of the fused posterior passes, as the last
 * posterior evaluation or E-step left them, to out (host).  *n_words is their length in 64-bit words; when it exceeds
 * max_words nothing is copied and the call still returns TEHMM_OK.  TEHMM_ERR_ARG when the batch holds no records.
 * TEHMM_ROWINDEX_REF=1 in the environment of an evaluation (test-only as well) builds the records with the plain
 * kernel that defines their layout; the default builder must produce the same bytes.  Records are cached per batch:
 * the knob is read at every evaluation and records built by the other kernel are rebuilt. */
int tehmm_debug_read_rowindex(tehmm_batch_t *batch, unsigned long long *out, int64_t max_words, int64_t *n_words);

#ifdef __cplusplus
}
#endif
#endif /* TEHMM_HIP_H */
