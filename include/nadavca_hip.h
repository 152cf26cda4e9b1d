/*
 * nadavca_hip.h — C ABI of libnadavca_hip.so, the MI355X (gfx950) engine behind
 * Nadavca's signal-to-reference alignment operators.
 *
 * This is the drop-in boundary for the reference's pybind11 module `nadavca.dtw`
 * (/root/reference/nadavca/dtw/dtwmodule.cpp:10-29; C++ declarations in
 * /root/reference/nadavca/dtw/dtw.h:6-18 and kmer_model.h:18-25).  Every entry
 * point below names the reference interface it replaces.  Plain pointers and
 * sizes only; the caller owns every buffer it passes, the library keeps nothing
 * past the call except what hangs off the opaque handles.
 *
 * Batched, flat ("CSR") argument layout.  A batch of n reads is described by
 *   signal      f64[ sig_off[n] ]      samples of read j: [sig_off[j], sig_off[j+1])
 *   reference   i32[ ref_off[n] ]      bases 0..alphabet-1
 *   ctx_before  i32[ cb_off[n] ]       k-mer context left of the reference part
 *   ctx_after   i32[ ca_off[n] ]       k-mer context right of it
 *   anchors     i32[ 2*anc_off[n] ]    rows (signal_index_in_slice, reference_index)
 *   *_off       i64[n+1]               exclusive prefix sums, off[0] = 0
 * which is the per-read argument list of the reference (signal, reference,
 * context_before, context_after, approximate_alignment) concatenated over reads.
 *
 * Two flavours of each operator:
 *   nvk_xxx_batch      host pointers   (uploads, runs and downloads in overlapped chunks: csrc/pipeline.hip)
 *   nvk_xxx_batch_dev  device pointers (inputs already resident in HBM; runs on the
 *                      context's HIP stream; results are complete on return)
 *
 * There is NO CPU fallback: without a usable HIP device every compute call
 * returns NVK_ERR_NO_DEVICE.
 */
#ifndef NADAVCA_HIP_H
#define NADAVCA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nvk_ctx nvk_ctx;     /* one per process/GPU: stream, workspaces, timers */
typedef struct nvk_model nvk_model; /* device-resident k-mer table, bound to a ctx */

/* call status */
enum {
  NVK_OK = 0,
  NVK_ERR_NO_DEVICE = -1,   /* no HIP device / runtime failure at init */
  NVK_ERR_INVALID = -2,     /* bad argument (see nvk_last_error) */
  NVK_ERR_HIP = -3,         /* a HIP call failed */
  NVK_ERR_UNSUPPORTED = -4, /* parameter outside the compiled range */
  NVK_ERR_NOMEM = -5
};

/* per-read status written by the batch operators */
enum {
  NVK_READ_OK = 0,
  NVK_READ_NO_PATH = 1,       /* reference: refine_alignment returns [] (dtw.cpp:211-213) */
  NVK_READ_BAD_INPUT = -1,    /* empty reference/signal, anchor outside the reference, a base code outside
                                 0..alphabet-1 in the reference or a context, offsets beyond total_* */
  NVK_READ_BAD_BAND = -2,     /* band_end < band_start for some row (reference: UB / length_error) */
  NVK_READ_TOO_WIDE = -3      /* the read's band is wider than the compiled kernels' on-chip rings hold
                                 (limits); the other reads of the batch are unaffected */
};

/* kernel ids for nvk_timing_read */
enum {
  NVK_K_PLAN = 0,        /* band + row-table planner */
  NVK_K_ALIGN = 1,       /* banded forward-backward + path search (refine_alignment) */
  NVK_K_ELL_SWEEP = 2,   /* prefix/suffix sweeps of estimate_log_likelihoods */
  NVK_K_ELL_HYP = 3,     /* per-base substitution hypotheses */
  NVK_K_EXPECTED = 4,    /* expected-level gather */
  NVK_K_CONSENSUS = 5,   /* normalise + strand flip + scatter-add */
  NVK_K_POSTERIOR = 6,   /* windowed posterior */
  NVK_K_RENORM = 7,      /* normalisation, per-event means, linear re-fit (align_signal's renorm loop) */
  NVK_K_METH = 8,        /* pattern occurrences and their scores (detect_meth) */
  NVK_K_SEED = 9,        /* the seed aligner: banded local alignment + traceback (nvk_seed_extend_*_dev), seed chains
                            (nvk_seed_chain_dev) */
  NVK_K_KMER = 10,       /* per-event and per-k-mer sample statistics of k-mer table training (nvk_kmer_*_dev) */
  NVK_K_ALLELE = 11,     /* per-site allele mixtures: rows and the per-position solve (nvk_allele_*_dev) */
  NVK_K_SITE = 12,       /* per-site event-level pile-up: rows and the per-key moments (nvk_site_*_dev) */
  NVK_K_COUNT = 13
};

const char *nvk_last_error(void); /* thread-local message of the last failing call */
int nvk_device_count(void);       /* number of visible HIP devices (0 if none) */

int nvk_ctx_create(int device, nvk_ctx **out);
void nvk_ctx_destroy(nvk_ctx *ctx);
int nvk_ctx_synchronize(nvk_ctx *ctx);
void *nvk_ctx_stream(nvk_ctx *ctx); /* the hipStream_t all kernels of this ctx run on */
/* number of reads processed concurrently by the sweep kernels (0 = automatic) */
int nvk_ctx_set_slots(nvk_ctx *ctx, int slots);

/* per-kernel HIP-event timing on the ctx stream (bench.py's roofline leg) */
int nvk_timing_enable(nvk_ctx *ctx, int on);
int nvk_timing_reset(nvk_ctx *ctx);
int nvk_timing_read(nvk_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
/* counters of the last batch call: total band cells C = sum_r W_r,
 * wavefront steps, and the workspace bytes the sweep kernels streamed */
int nvk_last_batch_stats(nvk_ctx *ctx, int64_t *band_cells, int64_t *wave_steps,
                         int64_t *spill_bytes);
/* reads of the last nvk_refine_alignment_batch[_dev] call that left the fast kernel's number range
 * and were recomputed by the exact kernel (results are the same either way; this is a cost figure) */
int nvk_last_retry_count(nvk_ctx *ctx, int64_t *n_reads);
/* PARITY CONTRACT of refine_alignment.  The reference decides every step of its path search with a strict
 * `>` between natural-log doubles (/root/reference/nadavca/dtw/node.cpp:52,72,82) that it produced with
 * a + log(1 + exp(b - a)) (probability.cpp:33-40).  This engine computes the same scores as scaled linear
 * numbers (2^-53 relative precision) and takes `a > b` only if a exceeds b by more than one ulp of the
 * reference's log value (relative margin |exponent| * 2^-52, xm::gt_tol), so that a plateau the reference
 * sees as flat resolves to the first maximum as it does there.  Every comparison whose two scores are closer
 * than the TIE MARGIN, 2^-24 RELATIVE (NVK_TIE_BITS in csrc/xmath.h), is recorded per read, in three classes:
 *   NVK_TIE_EXACT  the two scores are exactly equal.  Both sides resolve an exact tie the same way (no update,
 *                  the first maximum stays).
 *   NVK_TIE_ULP    different, but by no more than 64 of those ulp-sized margins (NVK_TIE_ULPS): the zone in
 *                  which the reference's OWN choice can hang on the rounding of its log-doubles — a flat
 *                  posterior plateau between two bases with the same k-mer level seen through rounding noise,
 *                  or an ill-conditioned arg-max.
 *   NVK_TIE_NEAR   further apart than that, still inside 2^-24 relative: both sides resolve the difference,
 *                  kept as a safety margin around the class above.
 * CONTRACT: a read with neither NVK_TIE_ULP nor NVK_TIE_NEAR has the reference's events exactly (asserted
 * read by read in tests/test_gpu_parity_full.py on randomised models, wide bands, homopolymer-rich references).
 * A read that carries such a bit and differs is an ARG-MAX OF THE REFERENCE'S PATH OBJECTIVE all the same: its
 * rows are a path the reference's search allows (bands, minimum event lengths, finite posteriors), and the sum
 * over DP rows of the log posterior boundary marginal (node.cpp:39-91) along it, evaluated in 80-bit arithmetic
 * by the CPU restatement (oracle/: orc_path_score), reaches that of the better of the reference's double and
 * long-double paths to within d * NVK_TIE_ULPS ulps of the reference's log score (d * 64 * 2^-52 * the largest
 * partial sum), d the number of DP rows at which the two paths differ: each tolerant comparison of the search
 * can cost at most one such zone, and each deviating decision leaves at least one differing row.  Proven, not
 * assumed: tests/fuzz_cases.py::classify_difference scores every differing read of the randomised campaigns
 * (tests/test_gpu_parity_full.py, tests/test_gpu_parity_scored.py) and every read of the census, which runs a named
 * case per built kernel variant and asserts through the launch report below that the variant ran
 * (tests/test_gpu_variant_census.py), and fails the suite on one that loses more; the largest deficit
 * measured is 2.5e-4 of that margin.
 * What the bits do NOT mean: that a flagged read differs.  Integer ADC samples repeat, so sequencer-shaped
 * data is full of equal and almost-equal path scores — the reference's own arithmetic meets ~25 exactly equal
 * and ~15 closer-than-2^-24 pairs of scores per config-2 read quantised to ADC steps (tests/dev/ref_tie_histogram.py)
 * — and almost every such read carries NEAR (and most ULP) bits; yet all 10 000 of them, and all 10 000 reads of
 * the int16 api_align_signal workload in both of align_signal's alignment passes, EQUAL the reference row for
 * row (the same test file; rates per class in DESIGN.md 2.1).  Every difference ever observed sits in a read
 * with the ULP bit, on a boundary between two bases with the same k-mer level or where the reference's
 * answer changes when it is recomputed in 80-bit long double.
 * Beside the three classes, nvk_last_tie_flags carries a structural mark,
 *   NVK_TIE_PLATEAU  two ADJACENT bases of the read have the same k-mer level (a homopolymer run of k+1 bases, or
 *                  a model with few levels): the boundary between their events is mathematically unidentifiable —
 *                  the posterior is exactly flat over a stretch of samples — and the reference places it by the
 *                  rounding noise of its log-doubles.  All but 24 of the 3 400 differing reads the randomised runs
 *                  ever produced differ only at such boundaries.  Not a tie class: it is known
 *                  from the sequence alone, is not counted by nvk_last_tie_count(s), and says nothing about the
 *                  rest of the read.
 *   nvk_last_tie_count    reads of the last nvk_refine_alignment_batch[_dev] call with a class bit set
 *   nvk_last_tie_counts   the same per class (a read may carry several bits)
 *   nvk_last_tie_flags    per read, the OR of its classes; out_flags i32[n_reads] (host), n_reads must be that
 *                         call's n_reads */
enum { NVK_TIE_EXACT = 1, NVK_TIE_NEAR = 2, NVK_TIE_ULP = 4, NVK_TIE_PLATEAU = 8 };
int nvk_last_tie_count(nvk_ctx *ctx, int64_t *n_reads);
int nvk_last_tie_counts(nvk_ctx *ctx, int64_t *n_exact, int64_t *n_near, int64_t *n_ulp);
int nvk_last_tie_flags(nvk_ctx *ctx, int64_t n_reads, int32_t *out_flags);
/* Cap, in bytes, on the device memory the sweep kernels take for their per-wave spill (the suffix rows of
 * the reads in flight: 512 B per wavefront step and resident wave).  0 (default): up to 60 % of the memory
 * that is free at the call.  Fewer waves run concurrently when the cap binds; results do not change.
 * The same cap bounds the traceback store of nvk_seed_extend_dev: when a batch's store is larger, its reads run in
 * chunks that fit (a single read larger than the cap runs on its own); results do not change. */
int nvk_ctx_set_workspace_limit(nvk_ctx *ctx, int64_t bytes);

/* LAUNCH REPORT: which compiled kernel variant the last call ran.  refine_alignment and the four log-likelihood
 * operators are served by families of template instantiations that the launchers pick from the batch's shape
 * (csrc/kernels_align3.hip: select_sweeps, csrc/kernels_align.hip: align_kernel<MEL>, csrc/kernels_ell.hip:
 * ell_dispatch); every nvk_refine_alignment_batch_dev, nvk_estimate_log_likelihoods_batch_dev and
 * nvk_estimate_{,joint_,edit_}hypotheses_batch_dev call clears the report of its ctx when it starts and adds one
 * record per launch class (not per chunk: `chunks` counts them).  Host stores only; nothing is read back for it.
 * Defined for these device-pointer calls only: the host-pointer entries (nvk_refine_alignment_batch, _submit,
 * nvk_estimate_log_likelihoods_batch) run their chunks on private lanes and leave the ctx with an EMPTY report.
 *   op        NVK_LAUNCH_SWEEP  a reverse/forward sweep pair of kernels_align3.hip
 *             NVK_LAUNCH_EXACT  align_kernel<mel> (kernels_align.hip), one record per class (narrow / wide skew)
 *             NVK_LAUNCH_ELL    ell_kernel<mel, lanes, kind> (kernels_ell.hip)
 *   mel       min event length, the template argument
 *   transitions  SWEEP, EXACT: transition rows on (SWEEP: the paired variant).  ELL: model_wobbling (a run-time flag)
 *   waves     SWEEP: waves per read, 1 or 4 (a team).  EXACT: 1.  ELL: lanes per hypothesis, 8 or 16
 *   period    SWEEP: rescale period in steps, 8, 16 or 32 (the template argument 1 << RSH).  Else 0
 *   kind      ELL: NVK_ELL_FULL / _LISTED / _JOINT / _EDIT.  EXACT: 1 = the retry launch behind the sweeps (it
 *             serves the reads they handed on: nvk_last_retry_count), 0 = the whole batch (NADAVCA_ALIGN_KERNEL=1).
 *             SWEEP: 0
 *   c         the largest skew the launch serves, after the fit into a CU's 160 KB of LDS: SWEEP, EXACT wide class:
 *             reads above it go to the exact kernel / get NVK_READ_TOO_WIDE; ELL: c_max, NVK_READ_TOO_WIDE above it
 *   H, SR     slots of the history ring and samples of the (per-wave) signal ring the launch was sized with
 *   lds_bytes dynamic LDS of the launch (SWEEP: of the forward launch, the larger of the pair)
 *   reads     reads of the launch class (EXACT retry: the reads of the class the launch scans for handed-on ones)
 *   chunks    launches (SWEEP: launch pairs) the class was served in
 * nvk_last_launches: up to `cap` records into out (host), *n_records = the number the call made (at most
 * NVK_LAUNCH_CAP are kept).
 * nvk_last_read_skews: per read of that call the planner's wavefront skew c and, for a read swept by a team of
 * waves, its team skew cw (else 0) — ONE copy of the ReadMeta table the call left on the device; n_reads must be
 * that call's n_reads, and a later call of any operator that plans reads on the ctx invalidates it (NVK_ERR_INVALID,
 * as nvk_last_tie_flags does).  out_c / out_cw: i32[n_reads] on the host, either may be NULL.
 * nvk_built_sweep_variants: the (mel, transitions, waves, period) combinations select_sweeps has a kernel pair for,
 * asked of select_sweeps itself over mel 0..7, transitions 0/1, waves 1..8, period 1..256: out i32[4 * cap],
 * *n_variants = how many there are.  The log-likelihood kernels are the full product mel 0..4 x lanes {8, 16} x the
 * four kinds (40) by construction of ell_dispatch's tables, the exact kernels mel 0..4 (5).
 * tests/test_gpu_variant_census.py runs a named smallest case (tests/variant_cases.py) per built variant, asserts
 * through this report that the case reached it and compares it with the CPU oracle. */
enum { NVK_LAUNCH_SWEEP = 1, NVK_LAUNCH_EXACT = 2, NVK_LAUNCH_ELL = 3 };
enum { NVK_ELL_FULL = 0, NVK_ELL_LISTED = 1, NVK_ELL_JOINT = 2, NVK_ELL_EDIT = 3 };
enum { NVK_LAUNCH_CAP = 8 };
typedef struct nvk_launch_rec {
  int32_t op, mel, transitions, waves, period, kind, c, H, SR, lds_bytes;
  int64_t reads, chunks;
} nvk_launch_rec;
int nvk_last_launches(nvk_ctx *ctx, int cap, nvk_launch_rec *out, int *n_records);
int nvk_last_read_skews(nvk_ctx *ctx, int64_t n_reads, int32_t *out_c, int32_t *out_cw);
int nvk_built_sweep_variants(int cap, int32_t *out, int *n_variants);

/* SELF-TEST of a helper no result can check.  The sweeps of csrc/kernels_align3.hip move their running scale by the
 * largest exponent the wave holds, taken with wave_max_i (csrc/wave.h: the maximum of the wave's 64 lanes in a scalar
 * register, on the DPP path).  A rescale by any common power of two is exact, so a wrong maximum changes no event —
 * at worst it hands a read to the exact kernel — and no comparison of results can see it.
 * nvk_selftest_wave_max: one small kernel in which wave w reduces in[w][0..63] with that very function and stores
 * out[w].  in: i32[n][64], out: i32[n], both DEVICE pointers; synchronous.  tests/test_gpu_wave_max.py compares it
 * with the host's maximum of each row. */
int nvk_selftest_wave_max(nvk_ctx *ctx, const int32_t *in, int64_t n, int32_t *out);

/* replaces dtw.KmerModel(k, central_position, alphabet_size, mean, sigma)
 * (dtwmodule.cpp:12-13, kmer_model.cpp:6-14).  mean/sigma: host f64[n], n = alphabet^k */
int nvk_model_create(nvk_ctx *ctx, int k, int central_position, int alphabet_size,
                     const double *mean, const double *sigma, int64_t n, nvk_model **out);
void nvk_model_destroy(nvk_model *model);
/* replaces KmerModel.get_k / get_central_position (dtwmodule.cpp:14-15) */
int nvk_model_info(const nvk_model *model, int *k, int *central_position, int *alphabet_size);

/* replaces KmerModel.get_expected_signal(reference, context_before, context_after)
 * (dtwmodule.cpp:16-18, kmer_model.cpp:32-42), batched.  out: f64[ref_off[n]] */
int nvk_expected_signal_batch(nvk_model *model, int64_t n_reads, const int32_t *reference,
                              const int64_t *ref_off, const int32_t *ctx_before,
                              const int64_t *cb_off, const int32_t *ctx_after,
                              const int64_t *ca_off, double *out);
int nvk_expected_signal_batch_dev(nvk_model *model, int64_t n_reads, int64_t total_ref,
                                  const int32_t *reference, const int64_t *ref_off,
                                  const int32_t *ctx_before, const int64_t *cb_off,
                                  const int32_t *ctx_after, const int64_t *ca_off, double *out);

/* replaces dtw.refine_alignment(signal, reference, context_before, context_after,
 * approximate_alignment, bandwidth, min_event_length, kmer_model, model_transitions)
 * (dtwmodule.cpp:24-28, dtw.cpp:133-228), batched.
 *   out_events  i32[2*ref_off[n]]  (event_start, event_end) per base, slice coordinates
 *   out_status  i32[n]             NVK_READ_*; for a read without a path its events are
 *                                  left untouched (the reference returns an empty list) */
int nvk_refine_alignment_batch(nvk_model *model, int64_t n_reads, const double *signal,
                               const int64_t *sig_off, const int32_t *reference,
                               const int64_t *ref_off, const int32_t *ctx_before,
                               const int64_t *cb_off, const int32_t *ctx_after,
                               const int64_t *ca_off, const int32_t *anchors,
                               const int64_t *anc_off, int bandwidth, int min_event_length,
                               int model_transitions, int32_t *out_events, int32_t *out_status);
/* device-pointer flavour: total_* are the host-known last entries of the offset arrays */
int nvk_refine_alignment_batch_dev(nvk_model *model, int64_t n_reads, int64_t total_signal,
                                   int64_t total_ref, int64_t total_anchors, const double *signal,
                                   const int64_t *sig_off, const int32_t *reference,
                                   const int64_t *ref_off, const int32_t *ctx_before,
                                   const int64_t *cb_off, const int32_t *ctx_after,
                                   const int64_t *ca_off, const int32_t *anchors,
                                   const int64_t *anc_off, int bandwidth, int min_event_length,
                                   int model_transitions, int32_t *out_events,
                                   int32_t *out_status);

/* PLAN ONCE, SWEEP AGAIN.  Before its sweeps a refine call plans the batch: bands, lane records, launch order and step
 * counts, about 3 % of a 10 000-read call, plus a round trip to the host that the sweeps wait for.  That plan is a
 * function of the read GEOMETRY only — n_reads, the three totals, sig_off, reference, ref_off, both contexts and their
 * offsets, anchors and anc_off, bandwidth, min_event_length, model_transitions and the model — and of no sample.  A
 * caller that aligns one resident batch again and again (align, re-fit the signal in place, align again) says so with
 * a token:
 *   nvk_plan_token_new   a fresh token: process-wide, monotonic, never 0.  Thread-safe.
 *   nvk_refine_alignment_batch_dev_keyed   nvk_refine_alignment_batch_dev with a token as its last argument.
 * CONTRACT: one token stands for ONE IMMUTABLE GEOMETRY.  Between two calls with the same token the arrays and scalars
 * listed above hold the same values at the same addresses; the samples behind `signal` (and the pointer itself) may
 * change freely, and so may the output arrays.  A caller that changes any of the geometry takes a new token.  The
 * addresses alone never identify a batch (an allocator gives the next batch of the same shape the same ones); they
 * are compared as a cross-check only.
 * A ctx holds at most one plan: that of the last keyed call that planned on it.  A keyed call whose token, model,
 * scalars, totals and addresses equal the held plan's sweeps from it: no planner and no order kernels are launched
 * (NVK_K_PLAN counts none), and nothing is copied or waited for before the sweeps are queued.  Any other call plans
 * as ever and, if its token is not 0, leaves its plan behind; that is never an error.  Token 0 — which is what
 * nvk_refine_alignment_batch_dev passes, and with it the lanes of the host-pointer entries — never reuses and leaves
 * no plan.  The held plan is dropped by whatever overwrites it: another refine call that plans, any of the
 * log-likelihood operators, a workspace of the plan that has to grow; a destroyed model's plan can never match again.
 * Results, status, tie flags, batch statistics and the launch report of a call that reused are those of one that
 * planned, bit for bit (tests/test_gpu_plan_reuse.py).
 * NADAVCA_PLAN_REUSE=0 (read at every call) makes every call plan.  NADAVCA_ALIGN_KERNEL=1 plans with the exact
 * kernel's row table; a plan made in one of the two modes serves only calls in that mode.
 *   nvk_last_plan_reused   *reused = 1 if the last refine call on the ctx swept from a held plan, else 0 */
uint64_t nvk_plan_token_new(void);
int nvk_refine_alignment_batch_dev_keyed(nvk_model *model, int64_t n_reads, int64_t total_signal,
                                         int64_t total_ref, int64_t total_anchors, const double *signal,
                                         const int64_t *sig_off, const int32_t *reference,
                                         const int64_t *ref_off, const int32_t *ctx_before,
                                         const int64_t *cb_off, const int32_t *ctx_after,
                                         const int64_t *ca_off, const int32_t *anchors,
                                         const int64_t *anc_off, int bandwidth, int min_event_length,
                                         int model_transitions, int32_t *out_events,
                                         int32_t *out_status, uint64_t plan_token);
int nvk_last_plan_reused(nvk_ctx *ctx, int *reused);

/* The same operator for a STREAM of batches (T_e2e of SURVEY.md 8d: host arrays in, host arrays out, the PCIe
 * copies hidden behind the kernels).  The reference pays its copy-in / copy-out around every call
 * (dtwmodule.cpp:19-28); here nvk_refine_alignment_submit uploads batch k+1 and returns at once with a ticket
 * while the kernels of batch k still run (a few lanes: private streams, workspaces and worker threads, made on
 * first use, csrc/pipeline.hip), and nvk_refine_alignment_wait(ticket) returns when that batch's events and
 * status are in the arrays given at submit.  All host arrays of a batch must stay valid and untouched from
 * submit until its wait returns (a later submit may deliver an earlier batch's results; its verdict is kept
 * for its wait).  out_tie_flags: i32[n_reads] for the per-read NVK_TIE_* bits, or NULL.  Tickets are per
 * context; wait for every ticket exactly once.  nvk_refine_alignment_batch itself runs its one batch through
 * the same lanes in growing chunks. */
int nvk_refine_alignment_submit(nvk_model *model, int64_t n_reads, const double *signal,
                                const int64_t *sig_off, const int32_t *reference,
                                const int64_t *ref_off, const int32_t *ctx_before,
                                const int64_t *cb_off, const int32_t *ctx_after,
                                const int64_t *ca_off, const int32_t *anchors,
                                const int64_t *anc_off, int bandwidth, int min_event_length,
                                int model_transitions, int32_t *out_events, int32_t *out_status,
                                int32_t *out_tie_flags, int64_t *ticket);
int nvk_refine_alignment_wait(nvk_model *model, int64_t ticket);

/* replaces dtw.estimate_log_likelihoods(signal, reference, context_before, context_after,
 * approximate_alignment, bandwidth, min_event_length, kmer_model, model_wobbling)
 * (dtwmodule.cpp:19-23, dtw.cpp:37-131), batched.
 *   out_ll      f64[alphabet*ref_off[n]]  row-major (base position, substituted base)
 *   out_status  i32[n] */
int nvk_estimate_log_likelihoods_batch(nvk_model *model, int64_t n_reads, const double *signal,
                                       const int64_t *sig_off, const int32_t *reference,
                                       const int64_t *ref_off, const int32_t *ctx_before,
                                       const int64_t *cb_off, const int32_t *ctx_after,
                                       const int64_t *ca_off, const int32_t *anchors,
                                       const int64_t *anc_off, int bandwidth,
                                       int min_event_length, int model_wobbling, double *out_ll,
                                       int32_t *out_status);
int nvk_estimate_log_likelihoods_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off,
    const int32_t *reference, const int64_t *ref_off, const int32_t *ctx_before,
    const int64_t *cb_off, const int32_t *ctx_after, const int64_t *ca_off,
    const int32_t *anchors, const int64_t *anc_off, int bandwidth, int min_event_length,
    int model_wobbling, double *out_ll, int32_t *out_status);

/* The same operator for a LIST of substitutions instead of all (alphabet-1)*R of a read (dtw.cpp:83-85,93-129):
 * same flat batch layout and leading arguments as nvk_estimate_log_likelihoods_batch_dev, device pointers.
 *   hyp_off     i64[n+1]        read j owns the hypotheses hyp_off[j] .. hyp_off[j+1], in any order, duplicates
 *                               allowed, possibly none; copied to the host and checked (starts at 0, never
 *                               decreases, ends at total_hyp, at most 2^31 - 1 per read; else NVK_ERR_INVALID)
 *   hyp_pos     i32[total_hyp]  base position p of the read, 0 .. R-1
 *   hyp_base    i32[total_hyp]  substituted base b, 0 .. alphabet-1; b == reference[p] is allowed and gives the
 *                               no-substitution total
 *   out_hyp     f64[total_hyp]  out_hyp[h] = what the full entry writes to out_ll[(ref_off[j] + p) * alphabet + b]
 *                               (dtw.cpp:93-129); the hypotheses that are not listed are never run
 *   out_total   f64[n]          the read's likelihood without a substitution (dtw.cpp:83-85), for every read that
 *                               ran, also one without hypotheses
 *   out_status  i32[n]          as the full entry; a read with a p or b outside its range gets NVK_READ_BAD_INPUT
 *                               before any table is indexed and the rest of the batch completes.
 *                               NVK_READ_NO_PATH: the values are the -inf the sweeps give.  Outputs of a read
 *                               with a negative status are left untouched.
 * Compiled limits as the full entry: min_event_length 0..4, k <= 14, alphabet <= 8, skew <= 62. */
int nvk_estimate_hypotheses_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off,
    const int32_t *reference, const int64_t *ref_off, const int32_t *ctx_before,
    const int64_t *cb_off, const int32_t *ctx_after, const int64_t *ca_off,
    const int32_t *anchors, const int64_t *anc_off, int bandwidth, int min_event_length,
    int model_wobbling, int64_t total_hyp, const int64_t *hyp_off, const int32_t *hyp_pos,
    const int32_t *hyp_base, double *out_total, double *out_hyp, int32_t *out_status);

/* The same for JOINT hypotheses: a hypothesis is a SET of substitutions (p_1, b_1) .. (p_m, b_m) of one read with
 * strictly ascending positions, scored as a whole.  Entries with b_i == reference[p_i] change nothing and are
 * dropped; if none remain the value is the read's no-substitution total (the listed operator's rule for
 * b == reference[p]).  Otherwise, with back = k - central - 1 and fwd = central, the rows
 * first = max(0, p_1 - back) .. last = min(R - 1, p_m + fwd) are re-run from prefix[first], every k-mer read from the
 * sequence with ALL substitutions applied, and closed exactly as dtw.cpp:116-126 closes a single substitution: the
 * closing wobble row on band `last` (the kept quirk), then the total against suffix[last + 1].  With one effective
 * substitution this is nvk_estimate_hypotheses_batch_dev's value, bit for bit.  The reference's counterpart: with
 * ref' = the read's reference with the substitutions 1 .. m-1 applied and b_m != reference[p_m], the value is the
 * entry [p_m, b_m] of EstimateLogLikelihoods on ref' — its prefix' rows between p_1 - back and p_m - back are the
 * same NextRow calls on the same bands as the hypothesis loop's interior rows (dtw.cpp:51-64 against 103-115), and
 * prefix[first] and suffix[last + 1] see none of the substituted bases.
 * Same flat batch layout and leading arguments as nvk_estimate_hypotheses_batch_dev, device pointers.
 *   hyp_off     i64[n+1]          read j owns the hypotheses hyp_off[j] .. hyp_off[j+1] (any order, duplicates
 *                                 allowed, possibly none)
 *   sub_off     i64[total_hyp+1]  hypothesis h owns the substitutions sub_off[h] .. sub_off[h+1], possibly none
 *                                 (the total).  Both offset arrays are copied to the host and checked (start at 0,
 *                                 never decrease, end at total_hyp / total_sub, at most 2^31 - 1 hypotheses per
 *                                 read; else NVK_ERR_INVALID)
 *   sub_pos     i32[total_sub]    base position of the read, 0 .. R-1, strictly ascending within a hypothesis
 *   sub_base    i32[total_sub]    substituted base, 0 .. alphabet-1 (a letter takes 3 bits of the kernel's item
 *                                 code: nvk_model_create builds no table of more than 8 letters, and this entry
 *                                 answers NVK_ERR_UNSUPPORTED for one)
 *   out_hyp     f64[total_hyp], out_total f64[n], out_status i32[n]: as the listed operator.  A read gets
 *                                 NVK_READ_BAD_INPUT before any table is indexed — its outputs left untouched, the
 *                                 rest of the batch completes — when one of its hypotheses has a position or base
 *                                 out of range, positions that do not strictly ascend, or effective substitutions
 *                                 that re-run more than 14 rows (last - first + 1 > 14, that is p_m - p_1 > 14 - k
 *                                 away from the read's ends: a hypothesis takes one DPP row of 16 lanes, two of
 *                                 which are not rows).
 * Hypotheses of at most 6 rows run 8 per wave step like the listed ones, the others 4 per step, in one launch
 * after one pair of sweeps per read.  Compiled limits otherwise as the full entry. */
int nvk_estimate_joint_hypotheses_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off,
    const int32_t *reference, const int64_t *ref_off, const int32_t *ctx_before,
    const int64_t *cb_off, const int32_t *ctx_after, const int64_t *ca_off,
    const int32_t *anchors, const int64_t *anc_off, int bandwidth, int min_event_length,
    int model_wobbling, int64_t total_hyp, const int64_t *hyp_off, int64_t total_sub,
    const int64_t *sub_off, const int32_t *sub_pos, const int32_t *sub_base, double *out_total,
    double *out_hyp, int32_t *out_status);

/* The same for EDIT hypotheses — insertions and deletions, which no substitution operator can express.  An edit
 * (p, d, s) of a read with reference ref[0..R) deletes ref[p .. p+d) and puts the i = len(s) letters of s in its
 * place: ref' = ref[:p] + s + ref[p+d:], of length R' = R - d + i; the contexts stay.  out_hyp[h] is the read's
 * likelihood under ref': the no-substitution total of EstimateLogLikelihoods (dtw.cpp:83-85) on ref'.
 * The band of ref' is NOT recomputed from anchors; it is the read's own band (bs, be) through an index map.  Boundary
 * row r' = 0 .. R' of ref' has the band
 *     (bs[r'], be[r'])                  for r' < p,
 *     (bs[p-1], be[p+d])                for p <= r' < p + i (the inserted rows),
 *     (bs[r'-i+d], be[r'-i+d])          for r' >= p + i,
 * which is monotone and never empty.  It equals what ComputeBandStarts / ComputeBandEnds (dtw.cpp:7-35) give for ref'
 * with the anchors behind the edit shifted by i - d whenever no anchor sits on a deleted base (for a pure insertion:
 * always); where a deleted base carries an anchor, the mapped band is the definition.
 * With back = k - central - 1 and fwd = central, only the rows first' = max(0, min(p - 1, p - back)) ..
 * last' = min(R' - 1, p + i - 1 + fwd) of ref' are re-run (k - 1 + i rows in the interior; row p - 1 is taken also when
 * back = 0, because the band of boundary row p changes), from the stored prefix[first'], every k-mer and band read
 * through the map, and closed against the stored suffix row last' + 1 - i + d.  The close differs from the
 * substitution operators': the closing wobble row between last' and last' + 1 lives on band last' + 1, where the prefix
 * sweep puts it (dtw.cpp:53-58), not on band last' (dtw.cpp:116-123) — the reference has no edit behaviour to
 * preserve, and closed this way the value is the true total of ref', so out_hyp[h] - out_total[j] is an unbiased
 * log-likelihood ratio.  The substitution operators keep their quirk.
 * Same flat batch layout and leading arguments as nvk_estimate_joint_hypotheses_batch_dev, device pointers.
 *   hyp_off     i64[n+1]          read j owns the hypotheses hyp_off[j] .. hyp_off[j+1] (any order, duplicates
 *                                 allowed, possibly none)
 *   edit_pos    i32[total_hyp]    p: 1 <= p, so a base of the read stays in front of the edit
 *   edit_del    i32[total_hyp]    d: 0 <= d <= 255 (the item code keeps d in 8 bits) and p + d <= R - 1, so a base
 *                                 stays behind it
 *   ins_off     i64[total_hyp+1]  hypothesis h inserts the letters ins_off[h] .. ins_off[h+1] of ins_base, possibly
 *                                 none.  Both offset arrays are copied to the host and checked (start at 0, never
 *                                 decrease, end at total_hyp / total_ins, at most 2^31 - 1 hypotheses per read; else
 *                                 NVK_ERR_INVALID)
 *   ins_base    i32[total_ins]    letters 0 .. alphabet-1 (3 bits of the item code each: NVK_ERR_UNSUPPORTED for a
 *                                 table of more than 8 letters, as the joint entry); at most 13 per hypothesis
 *   out_hyp     f64[total_hyp], out_total f64[n], out_status i32[n]: as the listed operator.  (d, i) = (0, 0) gives
 *                                 the read's total, bit-equal to out_total.  A read gets NVK_READ_BAD_INPUT before
 *                                 any table is indexed — its outputs left untouched, the rest of the batch completes
 *                                 — when one of its edits has p < 1, d < 0, d > 255, p + d > R - 1, a letter out of
 *                                 range or re-runs more than 14 rows (last' - first' + 1 > 14: a hypothesis takes one
 *                                 DPP row of 16 lanes, two of which are not rows).  NVK_READ_NO_PATH: the values are
 *                                 the -inf the sweeps give.
 * Hypotheses of at most 6 rows run 8 per wave step, the others 4 per step (with the packaged 6-mer table a one-base
 * deletion re-runs 5 rows and a one-base insertion 6: both 8 per step), in one launch after one pair of sweeps per
 * read.  Compiled limits otherwise as the full entry. */
int nvk_estimate_edit_hypotheses_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off,
    const int32_t *reference, const int64_t *ref_off, const int32_t *ctx_before,
    const int64_t *cb_off, const int32_t *ctx_after, const int64_t *ca_off,
    const int32_t *anchors, const int64_t *anc_off, int bandwidth, int min_event_length,
    int model_wobbling, int64_t total_hyp, const int64_t *hyp_off, const int32_t *edit_pos,
    const int32_t *edit_del, int64_t total_ins, const int64_t *ins_off, const int32_t *ins_base,
    double *out_total, double *out_hyp, int32_t *out_status);

/* replaces the Chunk score accumulation of ProbabilityEstimator
 * (/root/reference/nadavca/estimator.py:45-47,112-119,226-231): for every read j,
 *   ll' = (ll - ll[0][reference[0]]) / normalization_event_length,
 *   reverse strand: column b -> alphabet-1-b and rows flipped,
 *   acc[chunk_start[j] + p][b] += ll'[p][b],  coverage[chunk_start[j] + p] += 1.
 * ll/reference/ref_off as produced by nvk_estimate_log_likelihoods_batch(_dev).
 * Reads with status != 0 are skipped (status NULL: every read counts); positions outside [0, ref_len) are
 * dropped.  normalization_event_length is finite and not 0 (NVK_ERR_INVALID otherwise: a NaN would make every sum
 * NaN, an infinity every sum 0).  All pointers are device pointers; acc f64
 * [ref_len*alphabet] and coverage i64[ref_len] are accumulated into (not zeroed). */
int nvk_consensus_accumulate_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, int alphabet,
                                 const double *ll, const int32_t *reference,
                                 const int64_t *ref_off, const int64_t *chunk_start,
                                 const int32_t *reverse, const int32_t *status,
                                 double normalization_event_length, int64_t ref_len, double *acc,
                                 int64_t *coverage);

/* replaces ProbabilityEstimator._compute_posterior / _corrected_priors
 * (estimator.py:123-156) for n_segments independent groups of consecutive positions laid end to end:
 * segment s covers positions [seg_off[s], seg_off[s+1]); context windows never cross a segment border.
 * ll f64[len*alphabet], reference i32[len] (numerical bases), seg_off i64[n_segments+1],
 * out f64[len*alphabet]; device pointers. */
int nvk_posterior_segments_dev(nvk_ctx *ctx, int64_t len, int64_t n_segments, const int64_t *seg_off,
                               int alphabet, int k, double snp_prior, const double *ll,
                               const int32_t *reference, double *out);

/* ---- host steps adjacent to the path, on the device ------------------------ */

/* replaces Read.normalize_reads (/root/reference/nadavca/read.py:68-81) for n_groups independent
 * groups of samples laid end to end (group g = raw[grp_off[g] .. grp_off[g+1])):
 *   centre = median, scale = median |x - centre| (exact selections, the mean of the two middle
 *   values for an even count), out = clip((x - centre) / scale, -5, 5).
 * align_signal normalises every read on its own (one group per read, align_signal.py:54),
 * estimate_snps all reads together (one group, estimate_snps.py:61).  out may alias raw;
 * centre_scale f64[2*n_groups] receives (centre, scale) per group, or NULL.  Device pointers. */
int nvk_normalize_groups_dev(nvk_ctx *ctx, int64_t n_groups, const double *raw, const int64_t *grp_off,
                             double *out, double *centre_scale);

/* The same normalisation when the samples of the one group are SHARDED over several GPUs (estimate_snps takes
 * ONE median / MAD over all reads, estimate_snps.py:61, read.py:68-81; SURVEY.md 8e "caveat"): the exact
 * selection is a radix select over the order-preserving 64-bit key of a double, 8 passes of 8 bits, and only the
 * 256 counts of a pass have to cross ranks.  nvk_select_hist_dev counts, among this rank's x[0..n), the values
 * f(x) whose key agrees with `key_prefix` in the bits above pass `pass` (0 = most significant byte), by the byte
 * of that pass: hist256 u64[256] (device, overwritten).  mode 0: f(x) = x; mode 1: f(x) = |x - centre|.  The
 * caller sums the counts over the ranks (an all-reduce of 2 KB), picks the bucket holding the wanted rank and
 * extends the prefix (nadavca_amd/distributed.py: pooled_median).  nvk_normalize_apply_dev then writes
 * clip((x - centre) / scale, -5, 5); out may alias x.  Device pointers. */
int nvk_select_hist_dev(nvk_ctx *ctx, const double *x, int64_t n, int mode, double centre, uint64_t key_prefix,
                        int pass, uint64_t *hist256);
int nvk_normalize_apply_dev(nvk_ctx *ctx, const double *x, int64_t n, double centre, double scale, double *out);

/* replaces the per-event numpy.mean of align_signal.py:66-69 and read.py:85-86: for every base g of
 * every read, the mean of signal[sig_off[read] + events[2g] .. + events[2g+1]) with `events` as written
 * by nvk_refine_alignment_batch_dev (slice coordinates).  Summation in numpy's pairwise order, so the
 * result equals numpy.mean bit for bit; an empty event or a read with status != 0 gives NaN.
 * out_means f64[total_ref].  Device pointers; status may be NULL. */
int nvk_event_means_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                        const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                        const int32_t *status, double *out_means);

/* replaces scipy.stats.linregress(expected, means) and the rescale that follows it
 * (align_signal.py:71-73), per read:  slope = cov(x, y) / var(x), intercept = mean(y) - slope * mean(x),
 * then signal[sig_off[read] ..] = (signal - intercept) / slope in place.  Reads with status != 0 are
 * left alone.  out_fit f64[2*n_reads] receives (slope, intercept) so that the caller can apply the same
 * map to samples outside the slice, or NULL.  Device pointers. */
int nvk_linfit_rescale_dev(nvk_ctx *ctx, int64_t n_reads, const double *expected, const double *means,
                           const int64_t *ref_off, const int32_t *status, double *signal,
                           const int64_t *sig_off, double *out_fit);

/* replaces the FIT half of Read.tweak_signal_normalization (/root/reference/nadavca/read.py:83-93) for a
 * batch: per read, keep the events with |expected - means| <= 1, sort the pairs by (mean, level) as
 * numpy.lexsort((ys, xs)) does, and fit scipy.interpolate.splrep(xs, ys, s=len(xs)).  With that filter and that
 * s FITPACK's first trial — the least-squares cubic polynomial on the 8 knots [x0]*4 + [x_last]*4 — always meets
 * its acceptance test (the identity is a cubic and leaves sum (y-x)^2 <= m = s), so no knot is ever placed;
 * this restates that first pass of fpcurf.f operation for operation (coefficients equal scipy's bit for bit)
 * and VERIFIES the test per read.  means / expected: f64[total_ref], read j at [ref_off[j], ref_off[j+1]);
 * status int32[n_reads] or NULL: reads with status != 0 are not fitted.  Outputs per read: out_t f64[8] knots,
 * out_c f64[8] coefficients (4 + 4 zeros) — the layout nvk_splev_groups_dev takes with knot_off[j] = 8 j —
 * and out_fit int32: 0 fitted; 1 fewer than 4 usable events (no fit, placeholder spline written: the caller keeps
 * that read's samples); 2 FITPACK would go on to place knots (NaN input, all means equal: cannot happen under
 * the filter otherwise) — placeholder written, the caller fits that read with FITPACK itself.  Device pointers. */
int nvk_spline_fit_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *means,
                       const double *expected, const int64_t *ref_off, const int32_t *status, double *out_t,
                       double *out_c, int32_t *out_fit);

/* replaces scipy.interpolate.splev(x, (t, c, k)) — the evaluation half of
 * Read.tweak_signal_normalization (/root/reference/nadavca/read.py:94; the fit: nvk_spline_fit_dev) — for n_groups groups laid end to end: out[i] = spline_g(x[i]) for i in [grp_off[g], grp_off[g+1]),
 * spline g given by the knots t[knot_off[g] .. knot_off[g+1]) and as many coefficients c[...] as FITPACK
 * returns them, degree k (1..5), extrapolating outside the knots (ext = 0).  FITPACK's splev.f / fpbspl.f
 * restated operation for operation: results equal scipy's bit for bit.  out may alias x.  Device pointers. */
int nvk_splev_groups_dev(nvk_ctx *ctx, int64_t n_groups, const double *x, const int64_t *grp_off,
                         const double *t, const double *c, const int64_t *knot_off, int k, double *out);

/* replaces calculate_meth_scores + maxs3 of detect_meth (the reference's nadavca/detect_meth.py:21-65) for a batch,
 * in two passes: nvk_meth_count_dev counts, per read, the scorable occurrences of a pattern; the caller turns the
 * counts into offsets occ_off (exclusive prefix sum, occ_off[0] = 0) and nvk_meth_scores_dev writes them there.
 * Read j's reference part is reference[ref_off[j] .. ref_off[j+1]) (R_j bases 0..3, in the read's orientation),
 * with one event mean per base (means, as nvk_event_means_dev writes them: NaN for an empty event and for every
 * event of a read with status != 0) and one expected level per base (expected, nvk_expected_signal_batch_dev
 * without contexts).
 *   occurrence  p with pattern[0 .. pattern_len) == reference part [p .. p + pattern_len), p + pattern_len <= R_j;
 *               overlapping occurrences count (str.find restarts at pos + 1, detect_meth.py:35-40); pattern_len 0
 *               makes every position one; a pattern code outside 0..3 never matches
 *   scorable    p >= 5, p + 5 < R_j and none of the 11 means p-5 .. p+5 is NaN (detect_meth.py:42-50); a read
 *               with status != 0 has none (status may be NULL: every read counts)
 *   scores      per event i of the 11: -log(max(1e-50, erfc(z / sqrt 2))), z = |means - expected| / 0.35287208,
 *               i.e. 2 * Phi(-z) (cdf_scoring, detect_meth.py:23-26)
 *   aggregate   the largest of the nine sums (s[i] + s[i+1]) + s[i+2] (maxs3, detect_meth.py:63-65)
 * out_count i64[n_reads].  Occurrence k of read j (ascending position) goes to slot o = occ_off[j] + k:
 * out_pos[o] = p (position in the reference part), out_scores[11 o .. 11 o + 11), out_aggregate[o]; the outputs hold
 * occ_off[n_reads] entries; a read gets at most occ_off[j+1] - occ_off[j] of them.  The order is deterministic.
 * ref_off and occ_off are copied to the host and checked (start at 0, never decrease, ref_off ends at total_ref).
 * Device pointers. */
int nvk_meth_count_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int32_t *reference,
                       const int64_t *ref_off, const double *means, const int32_t *status, const int32_t *pattern,
                       int64_t pattern_len, int64_t *out_count);
int nvk_meth_scores_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int32_t *reference,
                        const int64_t *ref_off, const double *means, const double *expected, const int32_t *status,
                        const int32_t *pattern, int64_t pattern_len, const int64_t *occ_off, int64_t *out_pos,
                        double *out_scores, double *out_aggregate);

/* The extension stage of the seed aligner (nadavca_amd/seedalign.py): per read, a banded affine-gap local alignment
 * of the query against one strand of the reference, its traceback and the matched pairs.  Read j is
 * query[q_off[j] .. q_off[j+1]) (m_j base codes); the reference is given forward (ref_len = G codes); strand[j] 0 aligns
 * it to r = reference, 1 to r[x] = 3 - reference[G-1-x], -1 skips the read; diag[j] is the band centre d*.
 * Scores: match, mismatch, gap_open, gap_extend in 1..16 (a gap of length l costs gap_open + l * gap_extend).
 * A base code outside 0..3 on either side is a mismatch.  In int32, NEG = -2^30, O = gap_open + gap_extend,
 * X = gap_extend:
 *   cells   (i, j), 0 <= i < m, 0 <= j < G, d* - w <= j - i <= d* + w   (w = band, 1..256)
 *   D = (i > 0 && j > 0 ? H[i-1][j-1] : 0) + (q[i] == r[j] ? match : -mismatch)
 *   E = max(H[i][j-1] - O, E[i][j-1] - X) if (i, j-1) is a cell, else NEG     (a step along the reference)
 *   F = max(H[i-1][j] - O, F[i-1][j] - X) if (i-1, j) is a cell, else NEG     (a step along the read)
 *   best = max(D, E, F); best <= 0: H = 0, source START; else H = best, source DIAG if D == best, else E if
 *   E == best, else F.  E-extend bit of (i, j): E[i][j-1] - X > H[i][j-1] - O (opening wins a tie); F alike.
 *   end cell: largest H, then smallest i, then smallest j; its H is the score.  No cell at all: score 0, end -1.
 * A read whose score is >= min_score is traced back from its end cell, in state H:
 *   START: stop.  DIAG: emit (i, j) if q[i] == r[j], step to (i-1, j-1); stop if i or j was 0.
 *   E / F: go to state E / F at the same cell.  State E at (i, j): j -= 1, then stay in E if the E-extend bit of
 *   (i, j) before the step was set, else return to H.  State F likewise with i -= 1 and the F-extend bit.
 * out_hit i32[4 n_reads]: per read (score, i and j of the end cell, pair count).  The pairs, ascending, go to
 * out_pairs i32[2 total_query] as (i, j) at pair slots q_off[j] .. q_off[j] + count (a read emits at most m_j of
 * them): i in the read, j on the chosen strand.  A skipped read or one below min_score gets count 0 (its score and
 * end cell are still written; a skipped read's are 0, -1, -1).
 * The traceback store takes (2w + 1) / 2 bytes per cell (rounded up to whole strips of 64 rows); its size is bounded
 * by nvk_ctx_set_workspace_limit's cap.  q_off is copied to the host and checked (starts at 0, never decreases,
 * ends at total_query, no read above 2^26 bases); ref_len <= 2^30.  NVK_ERR_INVALID for bad arguments,
 * NVK_ERR_UNSUPPORTED for band > 256.  Device pointers. */
int nvk_seed_extend_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int32_t *query,
                        const int64_t *q_off, const int32_t *reference, int64_t ref_len, const int32_t *strand,
                        const int32_t *diag, int band, int match, int mismatch, int gap_open, int gap_extend,
                        int min_score, int32_t *out_hit, int32_t *out_pairs);

/* nvk_seed_extend_dev with a reference range per read, for a reference of several contigs laid end to end
 * (nadavca_amd/refset.py): ref_lo, ref_hi i32[n_reads], in coordinates of the strand read j is aligned to (on strand 1
 * contig [a, b) of the forward reference is [G - b, G - a)).  The same kernel and the same rules, with
 * the read's lo = ref_lo, hi = ref_hi:
 *   cells   (i, j), 0 <= i < m, lo <= j < hi, d* - w <= j - i <= d* + w
 * and lo wherever the rules above compare j with 0: D takes H[i-1][j-1] where i > 0 && j > lo; (i, j-1) is a cell only
 * for j > lo; the traceback's DIAG step stops if i was 0 or j was lo.  j is reported on the strand,
 * as above (not relative to ref_lo).  Equivalently: score, end cell, count and pairs are those of nvk_seed_extend_dev
 * on the reference cut to the range (for strand 1 the forward slice [G - ref_hi, G - ref_lo)) with diag - ref_lo, every
 * j moved back by ref_lo.  An empty range gives score 0, end -1, -1, no pairs.  With ref_lo = 0 and ref_hi = G for
 * every read the outputs are nvk_seed_extend_dev's.  ref_lo and ref_hi are copied to the host and checked like q_off:
 * for a read that is not skipped (strand != -1), ref_lo < 0, ref_hi > G or ref_lo > ref_hi is NVK_ERR_INVALID.  The
 * limit is G <= 2^30 over all contigs.  Device pointers. */
int nvk_seed_extend_bounded_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int32_t *query,
                                const int64_t *q_off, const int32_t *reference, int64_t ref_len, const int32_t *strand,
                                const int32_t *diag, const int32_t *ref_lo, const int32_t *ref_hi, int band, int match,
                                int mismatch, int gap_open, int gap_extend, int min_score, int32_t *out_hit,
                                int32_t *out_pairs);

/* The chaining stage of the seed aligner (seedalign.py with chain = 1): per read, the best collinear chain of its
 * seeds, and from it a band centre for every strip of 64 read rows, which nvk_seed_extend_path_dev follows.  THE
 * CONTRACT, integers only.  Read j has m_j = q_off[j+1] - q_off[j] bases, strand[j] as above, and the seeds
 * seed_off[j] .. seed_off[j+1] of (seed_i, seed_p): read k-mer i equals k-mer p of the read's strand,
 * 0 <= i < m_j, 0 <= p < 2^30, sorted ascending by (p, i) (none of this is checked: other values give other numbers,
 * never an access out of bounds).  Seeds are numbered t = 0, 1, .. in that order.  With k, w = band (1..256),
 * max_gap >= 1 and lookback in 1..64:
 *   predecessor  u of t: t - lookback <= u < t, and with di = i_t - i_u, dp = p_t - p_u:
 *                0 < di <= max_gap, 0 < dp <= max_gap, |dp - di| <= w
 *   score        f[t] = max(k, max over predecessors u of f[u] + min(di, dp, k) - |dp - di|); pred[t] is the u that
 *                reaches the maximum, the largest such u (the nearest seed) on a tie, and none when no predecessor's
 *                candidate exceeds k: a chain starts at t
 *   chain        ends at the t with the largest f, the smallest such t on a tie; its anchors are t, pred[t],
 *                pred[pred[t]], ..: i and p both strictly increase along it
 *   strip centre strip s = 0 .. ceil(m_j / 64) - 1 covers the rows 64 s .. 64 s + 63;
 *                strip_diag[strip_off[j] + s] = p - i of the anchor whose i is nearest to 64 s + 32, the smaller i
 *                on a tie
 * out_chain i32[2 n_reads]: per read (f of the chain's end, number of anchors).  A read without seeds, or with a strand
 * other than 0 or 1, gets (0, 0) and its entries of strip_diag are left as they were: the caller fills strip_diag
 * (i32[total_strips]) beforehand with the centre such a read is to get.  strip_off must be the running sum of
 * ceil(m_j / 64).  q_off, seed_off and strip_off are copied to the host and checked (start at 0, never decrease, end
 * at total_query / total_seeds / total_strips; no read above 2^26 bases or 2^26 seeds; the strip counts).  k in 1..16.
 * The kernel keeps f and pred in 8 bytes per seed of the ctx's workspace and is timed under NVK_K_SEED.
 * NVK_ERR_INVALID for bad arguments, NVK_ERR_UNSUPPORTED for band > 256.  Device pointers. */
int nvk_seed_chain_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int64_t *q_off,
                       const int32_t *strand, int64_t total_seeds, const int64_t *seed_off, const int32_t *seed_i,
                       const int32_t *seed_p, int k, int band, int max_gap, int lookback, int64_t total_strips,
                       const int64_t *strip_off, int32_t *strip_diag, int32_t *out_chain);

/* nvk_seed_extend_dev with a band that follows a path: the band of row i of read j is centred on
 * d(i) = strip_diag[strip_off[j] + i / 64] instead of the read's one diag[j] (strip_off, strip_diag and total_strips as
 * in nvk_seed_chain_dev; any int32 is a valid centre).  The same kernel body and the same rules, with
 *   cells   (i, j), 0 <= i < m, 0 <= j < G, d(i) - w <= j - i <= d(i) + w
 * and every "is a cell" of the rules — in E, in F and in what the traceback may stand on — meaning a cell of that
 * row's own band.  D = (H[i-1][j-1] if (i-1, j-1) is a cell, else 0) + (q[i] == r[j] ? match : -mismatch); with one
 * centre per read (i-1, j-1) is a cell whenever i > 0 and j > 0, so this is the rule above.  Where two strips' bands
 * share no diagonal, no cell of the second has a neighbour in the first, and alignments start afresh there.  The
 * traceback's DIAG step from (i, j) ends the walk where (i-1, j-1) is not a cell (its D took 0 from there).  With
 * every centre of read j equal to d the outputs are those of nvk_seed_extend_dev with diag[j] = d.
 * ref_lo, ref_hi: both NULL — the whole strand — or both i32[n_reads], and then the bounded rules of
 * nvk_seed_extend_bounded_dev apply as well, with its checks.  The traceback store, its size and the chunking under
 * nvk_ctx_set_workspace_limit's cap are nvk_seed_extend_dev's.  strip_off is copied to the host and checked as
 * nvk_seed_chain_dev checks it.  NVK_ERR_INVALID for bad arguments (one of ref_lo / ref_hi NULL among them),
 * NVK_ERR_UNSUPPORTED for band > 256.  Device pointers. */
int nvk_seed_extend_path_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int32_t *query,
                             const int64_t *q_off, const int32_t *reference, int64_t ref_len, const int32_t *strand,
                             int64_t total_strips, const int64_t *strip_off, const int32_t *strip_diag,
                             const int32_t *ref_lo, const int32_t *ref_hi, int band, int match, int mismatch,
                             int gap_open, int gap_extend, int min_score, int32_t *out_hit, int32_t *out_pairs);

/* The M-step of k-mer table training (nadavca_amd/kmer_train.py: estimate_kmer_model): per-k-mer sample statistics
 * over the final events of an aligned batch.  THE CONTRACT.  Inputs are one batch in the flat layout above: signal /
 * sig_off (the windows), events i32[2 total_ref] in slice coordinates as nvk_refine_alignment_batch_dev writes them,
 * per-read status, reference / ref_off, ctx_before / cb_off, ctx_after / ca_off, and k, central, alphabet, trim >= 0.
 *   counted event  base g of read j (0 <= g < R_j) with status[j] == 0 (status may be NULL: every read counts),
 *                  trim <= g < R_j - trim, a non-empty event after clamping start and end to 0 .. N_j (as
 *                  nvk_event_means_dev does), and a k-mer window wholly inside the extended sequence
 *                  ctx_before ++ reference part ++ ctx_after:  -len(cb_j) <= g - central  and
 *                  g - central + k - 1 < R_j + len(ca_j).  No base is read as 0 (unlike the expected levels).  A window
 *                  holding a code outside 0..alphabet-1 is not counted (refine_alignment refuses such reads anyway).
 *   key            id = sum_m b_m * alphabet^(k-1-m), b_m the extended-sequence base at g - central + m (the indexing
 *                  of the packaged table and of synthetic.kmer_ids)
 *   order          E_id = the counted events with key id in batch order (read ascending, then g ascending)
 *   pass 1         s_e = np.sum(x[a:b]) (numpy's pairwise order), n_e = b - a;  per k-mer S = np.sum of the s_e of
 *                  E_id gathered into one f64 array, N = sum n_e (int64), e = |E_id|; the caller takes m = S / N
 *   pass 2         q_e = np.sum(d * d), d = x[a:b] - m_id (a rounded subtraction, a rounded square: the library is
 *                  built with -ffp-contract=off);  per k-mer Q = np.sum of the q_e of E_id; sigma = sqrt(Q / N)
 * Every floating-point sum is a kernel's loop in numpy's order, with no atomics: the results equal numpy's bit for bit
 * and are the same on every run.
 * nvk_kmer_event_stats_dev writes per event (index ref_off[j] + g): out_key i64 (-1 when not counted), out_len i64
 * (n_e, 0 when not counted) and out_val f64 (0 when not counted): s_e when level is NULL, else q_e against
 * level[key] (f64[alphabet^k], device).  k >= 1, 0 <= central < k, alphabet >= 1, alphabet^k <= 2^31, trim >= 0;
 * ref_off, sig_off, cb_off and ca_off are copied to the host and checked (start at 0, never decrease, ref_off ends at
 * total_ref).
 * nvk_kmer_reduce_dev: key i64[n_events] is the events' keys sorted ascending by a STABLE sort, val f64 and len i64
 * [n_events] the events' values and lengths gathered into the same order; for every id in 0 .. n_kmers it writes
 * out_sum f64 = np.sum of val over the id's run of keys, out_samples i64 = the sum of their len, out_events i64 =
 * their number (0, 0, 0 where none was counted; keys outside 0 .. n_kmers are skipped).  n_kmers <= 2^31.
 * NVK_ERR_INVALID for bad arguments or offsets.  Device pointers. */
int nvk_kmer_event_stats_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                             const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                             const int32_t *reference, const int32_t *ctx_before, const int64_t *cb_off,
                             const int32_t *ctx_after, const int64_t *ca_off, const int32_t *status, int k, int central,
                             int alphabet, int trim, const double *level, int64_t *out_key, double *out_val,
                             int64_t *out_len);
int nvk_kmer_reduce_dev(nvk_ctx *ctx, int64_t n_events, int64_t n_kmers, const int64_t *key, const double *val,
                        const int64_t *len, double *out_sum, int64_t *out_samples, int64_t *out_events);

/* The M-step of modified-base table training (nadavca_amd/mod_train.py: estimate_mod_model): weighted per-k-mer sample
 * statistics over the final events of an aligned batch whose reference is CANONICAL, for the k-mers that hold the
 * modified base.  THE CONTRACT.  The library is built with -ffp-contract=off: every expression below is a rounded
 * operation in the order written.  Inputs are those of nvk_kmer_event_stats_dev, and
 *   sites          per read j its sites site_off[j] .. site_off[j+1] (i64[n_reads + 1], ending at n_sites): site_pos
 *                  i32 (a base of the reference part, strictly ascending within a read, inside [0, R_j)) and site_gamma
 *                  f64 in [0, 1], the probability that the read carries mod_code there.  Order and ranges are the
 *                  caller's promise; whatever the arrays hold, nothing outside them or outside a base's rows is touched.
 *   level          f64[alphabet^k], the current means; 0 <= mod_code < alphabet
 *   rows of base g its window is [g - central, g - central + k); m = the number of the read's sites inside it.  m == 0 or
 *                  m > 4: no rows (the bases with m > 4 are counted into *windows_skipped).  Otherwise 2^m - 1 rows, one
 *                  per non-empty subset `mask` in ascending mask, bit t of mask = the window's t-th site in ascending
 *                  position.  The number of rows does not depend on the event.
 *   counted event  exactly as nvk_kmer_event_stats_dev counts it (trim, the window inside the contexts, a non-empty
 *                  event after clamping, every code in range, status[j] == 0 or status NULL).  The rows of an event
 *                  that is not counted are (-1, 0.0, 0.0, 0.0, 0.0).
 *   values         for a counted event over the samples x[s:e], n = (double)(e - s): key0 = the window's k-mer id, c0 =
 *                  level[key0], a = sum (x[i] - c0) and b = sum (x[i] - c0) * (x[i] - c0), each an ascending loop from
 *                  0.0, once per event.  Per mask: key = the id with mod_code at the mask's sites; d = c0 - level[key];
 *                    sd = a + n * d                            (the sum of x - level[key])
 *                    sq = b + (2.0 * d) * a + (n * d) * d      (the sum of its squares)
 *                    w  = 1.0, then for t ascending over the window's sites  w = w * gamma_t  if bit t of mask is set,
 *                         else  w = w * (1.0 - gamma_t)
 *                  and the row is (key, w, n, sd, sq).
 * nvk_mod_kmer_rows_dev is called twice, as nvk_meth_count_dev / nvk_meth_scores_dev are.  With out_key and out_val NULL
 * it writes out_count i64[total_ref], the rows of every base (events, level and row_off are not read).  The caller forms
 * row_off i64[total_ref + 1] by a cumulative sum, n_rows = its end, and calls again with out_key i64[n_rows] and out_val
 * f64[4 n_rows] (w, n, sd, sq per row): base g of read j fills exactly [row_off[ref_off[j] + g], row_off[ref_off[j] + g +
 * 1)).  Where that range is not inside 0 .. n_rows or its width is not the base's row count, nothing is written for the
 * base, a device flag is raised (an integer atomic OR) and the entry returns NVK_ERR_INVALID.  windows_skipped is a HOST
 * pointer (may be NULL), written by both calls.  ref_off, site_off, sig_off, cb_off and ca_off are copied to the host and
 * checked (start at 0, never decrease, ref_off ends at total_ref, site_off at n_sites).
 * nvk_mod_kmer_reduce_dev: val f64[4 n_rows] is the rows gathered into the STABLE ascending order of their keys; run_off
 * i64[n_keys + 1] the runs of the distinct keys >= 0 in it: run_off[0] = the number of rows with a key < 0 (they come
 * first and are skipped), run_off[n_keys] = n_rows, never decreasing (copied to the host and checked).  Per run, over its
 * rows 0 .. c-1 in order, four sums W = sum w, Nw = sum w * n, Sd = sum w * sd, Sq = sum w * sq, each
 *   64 partial sums starting at 0.0, row i added to sum i mod 64 in ascending i, then combined by the butterfly
 *   p[l] = p[l] + p[l xor d] for d = 32, 16, 8, 4, 2, 1 (nvk_site_moments_dev's order).
 * out_sum f64[4 n_keys] = (W, Nw, Sd, Sq) per run, out_rows i64[n_keys] = c; every entry is written.  The caller takes
 * mean = level[key] + Sd / Nw and variance = Sq / Nw - (Sd / Nw)^2.
 * No floating-point atomics: the same bits on every run.  The launches are timed under NVK_K_KMER.  k, central, alphabet
 * and trim as for nvk_kmer_event_stats_dev; n_keys == 0 launches nothing.  NVK_ERR_INVALID for bad arguments or offsets;
 * a data pointer may be NULL only where its array is empty.  Device pointers but windows_skipped. */
int nvk_mod_kmer_rows_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                          const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                          const int32_t *reference, const int32_t *ctx_before, const int64_t *cb_off,
                          const int32_t *ctx_after, const int64_t *ca_off, const int32_t *status, int k, int central,
                          int alphabet, int trim, int64_t n_sites, const int64_t *site_off, const int32_t *site_pos,
                          const double *site_gamma, int mod_code, const double *level, int64_t n_rows,
                          const int64_t *row_off, int64_t *out_count, int64_t *out_key, double *out_val,
                          int64_t *windows_skipped);
int nvk_mod_kmer_reduce_dev(nvk_ctx *ctx, int64_t n_rows, int64_t n_keys, const double *val, const int64_t *run_off,
                            double *out_sum, int64_t *out_rows);

/* Per-site allele mixtures (nadavca_amd/allele_fractions.py: estimate_allele_fractions_batch): which share of the reads
 * that cover a reference position carries a base other than the reference's.  THE CONTRACT.  Take a global reference
 * position P with reference base r = ref_codes[P], and a base b != r.
 *   covering reads  the reads i with status[i] == 0 (status may be NULL: every read counts) whose reference part
 *                   covers P, in ascending read index
 *   per-read value  d_i = (ll_i[p, c] - ll_i[0, reference_i[0]]) / event_length, with (p, c) the read-frame row and
 *                   column of (P, b) as nvk_consensus_accumulate_dev maps them: a forward read has p = P - chunk_start,
 *                   c = b; a reverse read p = R - 1 - (P - chunk_start), c = alphabet - 1 - b.  The shift is the read's
 *                   total without a substitution.  d_i may be -inf.
 *   likelihood      L(f) = sum_i t(f, d_i);  t(f, d) = d + log(f + (1 - f) exp(-d)) for d > 0, else
 *                   log((1 - f) + f exp(d));  L(0) = 0.  exp(d) is never formed for a positive d.
 *   derivative      g(f) = sum_i u(f, d_i);  u(f, d) = (1 - exp(-d)) / (exp(-d) (1 - f) + f) for d > 0, else
 *                   (exp(d) - 1) / (1 + f (exp(d) - 1));  g does not increase on [0, 1].
 *   estimate        f^ = 0 unless g(0) > 0;  f^ = 1 if g(1) >= 0;  otherwise 52 bisection steps on [0, 1] (lo = m when
 *                   g(m) > 0, else hi = m) and f^ = (lo + hi) / 2
 *   outputs         per (P, b): fraction = f^, lrt = 2 L(f^) (0 when f^ = 0), ll_half = L(1/2), ll_full = L(1) =
 *                   sum_i d_i (the consensus sum when event_length is the configuration's normalization_event_length);
 *                   per P: coverage.  At b = r, where the coverage is 0, and where r is outside 0 .. alphabet-1, the
 *                   four values are 0.
 * nvk_allele_rows_dev takes nvk_consensus_accumulate_dev's inputs and event_length (> 0, finite) and writes, per
 * read-major row g = ref_off[i] + p: out_key i64[total_ref] = P, or -1 for a read with status != 0, a position outside
 * [0, ref_len), a read whose shift is not finite and a read whose reference[0] is outside 0 .. alphabet-1; out_val
 * f64[total_ref * alphabet] = the row's d in FORWARD columns (0 where the key is -1).  ref_off is copied to the host and
 * checked (starts at 0, never decreases, ends at total_ref).
 * nvk_allele_solve_dev: key i64[n_rows] is the rows' keys sorted ascending by a STABLE sort (keys < 0 come first and are
 * skipped, keys >= ref_len are skipped too), val f64[n_rows * alphabet] the rows gathered into the same order,
 * ref_codes i32[ref_len]; it writes out_fraction, out_lrt, out_ll_half, out_ll_full f64[ref_len * alphabet] and
 * out_coverage i64[ref_len], every entry.  Sums run over a position's rows in key order, 64 interleaved partial sums
 * (row j of the position goes to sum j mod 64) that a fixed butterfly adds up: no atomics, the same bits on every run;
 * L(f) is evaluated as (the sum of the positive d_i) + (the sum of the logarithms).  2 <= alphabet <= 8.
 * NVK_ERR_INVALID for bad arguments or offsets; a data pointer may be NULL only where its array is empty.  Device
 * pointers. */
int nvk_allele_rows_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, int alphabet, const double *ll,
                        const int32_t *reference, const int64_t *ref_off, const int64_t *chunk_start,
                        const int32_t *reverse, const int32_t *status, double event_length, int64_t ref_len,
                        int64_t *out_key, double *out_val);
int nvk_allele_solve_dev(nvk_ctx *ctx, int64_t n_rows, int64_t ref_len, int alphabet, const int64_t *key,
                         const double *val, const int32_t *ref_codes, double *out_fraction, double *out_lrt,
                         double *out_ll_half, double *out_ll_full, int64_t *out_coverage);

/* Phasing of heterozygous sites and haplotype tags of reads (nadavca_amd/phase.py: phase_reads_batch).  THE CONTRACT.
 * The library is built with -ffp-contract=off: every expression below is a rounded operation in the order written.
 *   sites      s = 0 .. S-1, each a global position P_s (strictly ascending) and ONE alternative base b_s, chosen by
 *              the caller on the host
 *   evidence   e_is = min(max(d_is, -clip), clip), d_is the value nvk_allele_rows_dev writes for (read i, P_s, forward
 *              column b_s); -inf (and a value that is not a number) gives -clip.  Read i has evidence at s only where
 *              the key of its read-major row of P_s equals P_s.
 *   links      for s >= 1 with chain_s != 0: over the reads with evidence at both s - 1 and s (the shared reads), in
 *              ascending read index, link_s = sum [ lae(e1 + e2, 0) - lae(e1, e2) ], lae(a, b) = max(a, b) +
 *              log1p(exp(-|a - b|)): the log-likelihood ratio of "both alternatives on one haplotype" against "on
 *              different ones" with the read's haplotype summed out at 1/2 : 1/2.  shared_s = their number.  The sum
 *              runs over the rows of site s in key order, 64 interleaved partial sums (row j of the site goes to sum
 *              j mod 64, ascending j; a row that is not shared adds +0.0) which wave_sum's butterfly adds up.  Site 0
 *              and every site with chain_s == 0 (the caller clears it at a contig's first site) get link 0, shared 0.
 *   blocks     (integer work, done by the caller on the device) s is joined to s - 1 iff chain_s, shared_s >=
 *              min_shared and |link_s| >= min_link; otherwise it opens a block.  block_s = the index of the block's
 *              first site.  sigma = +1 there, then sigma_s = sigma_{s-1} * (link_s > 0 ? +1 : -1): +1 says that the
 *              alternative of s lies on the haplotype that carries the alternative of the block's first site,
 *              haplotype 1 of the block.
 *   tag        per read, its sites with evidence in ascending s; those of one block form a run with H = the left to
 *              right double sum of sigma_s * e_is starting from 0.0.  The read's block is the run with the largest |H|,
 *              the first on ties: read_block (-1 for a read without a site), read_llr = H, read_sites = the length of
 *              that run.  Haplotype 1 if H > 0, 2 if H < 0, else none.
 *   vote       per site, leave-one-out: over the site's rows in key order whose read has read_block == block_s,
 *              h = read_llr_i - sigma_s * e_is; rows with h == 0 do not count; vote_s = sum sign(h) * e_is in the
 *              64-partial order of the links (a row that does not count adds +0.0); n_agree / n_against = the counted
 *              rows with sign(h) * sigma_s * e_is above / below 0.
 *   refinement (the caller's loop) `rounds` times: tag, vote, flip every sigma_s with vote_s * sigma_s < 0 at once,
 *              then multiply every block by its first site's sigma; a last tag and vote give the outputs.  Blocks are
 *              neither merged nor split.
 * The site entries work on the rows in STABLE key order as nvk_allele_solve_dev takes them: val f64[n_rows * alphabet],
 * row_read i64[n_rows] the read index of every sorted row (ascending inside a site because the sort is stable), and per
 * site its range of rows site_lo .. site_hi i64[n_sites] (inside 0 .. n_rows, hi >= lo), site_alt i32 in
 * 0 .. alphabet-1 (a site with another value gets zeros).  nvk_phase_links_dev: chain i32[n_sites]; writes out_link
 * f64 and out_shared i64, every entry.  nvk_phase_votes_dev: site_block i64, site_sigma i32 (+1 / -1), read_block i64
 * and read_llr f64 as nvk_phase_tag_dev wrote them (row_read indexes them); writes out_vote f64, out_agree and
 * out_against i64, every entry.
 * nvk_phase_tag_dev works on the READ-MAJOR key and val of nvk_allele_rows_dev with that call's ref_off (copied to the
 * host and checked: starts at 0, never decreases), chunk_start and reverse, and site_pos i64[n_sites]: a read's sites are
 * those with chunk_start <= P_s < chunk_start + R, the row of P_s is ref_off[i] + p with p = P_s - chunk_start for a
 * forward read and R - 1 - (P_s - chunk_start) for a reverse one; forward columns need no flip.  It writes out_block
 * i64, out_llr f64 and out_sites i64 [n_reads], every entry.
 * No atomics: the same bits on every run.  The launches are timed under NVK_K_ALLELE.  n_sites == 0 launches nothing
 * (and writes nothing).  2 <= alphabet <= 8, 0 < clip < inf.  NVK_ERR_INVALID for bad arguments or offsets or a NULL
 * array.  Device pointers. */
int nvk_phase_links_dev(nvk_ctx *ctx, int64_t n_sites, int alphabet, const int64_t *site_lo, const int64_t *site_hi,
                        const int32_t *site_alt, const int32_t *chain, const int64_t *row_read, const double *val,
                        double clip, double *out_link, int64_t *out_shared);
int nvk_phase_tag_dev(nvk_ctx *ctx, int64_t n_reads, int64_t n_sites, int alphabet, const int64_t *ref_off,
                      const int64_t *chunk_start, const int32_t *reverse, const int64_t *key, const double *val,
                      const int64_t *site_pos, const int32_t *site_alt, const int64_t *site_block,
                      const int32_t *site_sigma, double clip, int64_t *out_block, double *out_llr, int64_t *out_sites);
int nvk_phase_votes_dev(nvk_ctx *ctx, int64_t n_sites, int alphabet, const int64_t *site_lo, const int64_t *site_hi,
                        const int32_t *site_alt, const int64_t *site_block, const int32_t *site_sigma,
                        const int64_t *row_read, const double *val, const int64_t *read_block, const double *read_llr,
                        double clip, double *out_vote, int64_t *out_agree, int64_t *out_against);

/* Phasing across weak sites (phase_reads_batch with span > 1; csrc/kernels_phase.hip).  THE CONTRACT, in the terms
 * of the phasing contract above.
 *   span links nvk_phase_span_links_dev: for site s and w = 1 .. span with s - w >= site_first_s, out_link[s * span +
 *              w - 1] and out_shared[s * span + w - 1] are exactly the link and shared of the contract above taken between
 *              the sites s - w and s (e1 at s - w, e2 at s).  site_first i64[n_sites]: the index of the first site of
 *              s's contig (or of whatever stretch of sites the caller allows links inside); it takes the place of
 *              chain.  The sum runs over the rows of site s in key order, row j into partial sum j mod 64, a row that is
 *              not shared adds +0.0, and the partials are added by wave_sum's butterfly.  Every other entry is 0, and
 *              every entry of out_link f64[n_sites * span] and out_shared i64[n_sites * span] is written.  Column w = 1
 *              therefore has the bits of nvk_phase_links_dev wherever chain_s != 0.  1 <= span <= 8; the other argument
 *              rules are those of nvk_phase_links_dev.
 *   forest     (integer work, done by the caller on the device: device.phase_forest) candidate w of site s qualifies
 *              when s - w >= site_first_s, shared >= min_shared and |link| >= min_link.  parent_s = s - w*, w* the
 *              qualifying candidate with the largest |link|, the smallest w on ties; -1 without one.  block_s = the
 *              root of s, sigma_s = the product of (link > 0 ? +1 : -1) along the path to it.  Greedy: every site takes
 *              its strongest earlier neighbour; this is no maximum spanning tree.  A block is no interval of sites any
 *              more: a site without a qualifying link stays a singleton inside the block that its neighbours form.
 *   tag blocks nvk_phase_tag_blocks_dev, the arguments of nvk_phase_tag_dev, ANY block array: per read, for every
 *              block b that owns at least one of the read's sites with evidence, H_b = the left to right double sum of
 *              sigma_s * e_is over those sites in ascending s, starting from 0.0.  The read's block is the one with
 *              the largest |H_b|, the smallest block index on ties; read_llr = that H, read_sites = the number of its
 *              sites, -1 / 0 / 0 for a read without a site.  Where every block is an interval of sites labelled by its
 *              first site this is nvk_phase_tag_dev's answer bit for bit.
 *   vote, refinement: as above (nvk_phase_votes_dev serves any block array; "its first site" is the root).
 * No atomics: the same bits on every run.  The launches are timed under NVK_K_ALLELE.  n_sites == 0 launches nothing
 * (and writes nothing).  NVK_ERR_INVALID for bad arguments or offsets or a NULL array.  Device pointers. */
int nvk_phase_span_links_dev(nvk_ctx *ctx, int64_t n_sites, int span, int alphabet, const int64_t *site_lo,
                             const int64_t *site_hi, const int32_t *site_alt, const int64_t *site_first,
                             const int64_t *row_read, const double *val, double clip, double *out_link,
                             int64_t *out_shared);
int nvk_phase_tag_blocks_dev(nvk_ctx *ctx, int64_t n_reads, int64_t n_sites, int alphabet, const int64_t *ref_off,
                             const int64_t *chunk_start, const int32_t *reverse, const int64_t *key, const double *val,
                             const int64_t *site_pos, const int32_t *site_alt, const int64_t *site_block,
                             const int32_t *site_sigma, double clip, int64_t *out_block, double *out_llr,
                             int64_t *out_sites);

/* Per-site modification frequencies over sets of rows (nadavca_amd/phase_mods.py: phase_mods_batch,
 * mod_site_frequencies).  THE CONTRACT.  The library is built with -ffp-contract=off: every expression below is a
 * rounded operation in the order written.
 *   rows       val f64[n_rows]: one log-likelihood ratio d per row ("modified" against "canonical", as call_mods_batch
 *              writes it), in the caller's order; group i32[n_rows], or NULL: every row is group 0
 *   sites      s = 0 .. n_sites-1, each a range of rows site_lo[s] .. site_hi[s] (i64, inside 0 .. n_rows, hi >= lo; a
 *              range that leaves 0 .. n_rows is cut to it, so no call reads outside val)
 *   sets       q = 0 .. n_sets-1 (1 <= n_sets <= 8), each a mask set_mask[q] (u32) over the groups: set q of a site holds
 *              the site's rows whose group g is in 0 .. 31 with bit g of set_mask[q] set.  A row whose d is not a number
 *              and a row whose group is outside 0 .. 31 are in no set.
 *   value      e = min(max(d, -clip), clip): -inf gives -clip, +inf gives +clip
 *   estimate   per (site, set), over the values of the set's rows: t, u, L(f) = sum t(f, e_i), g(f) = sum u(f, e_i) and
 *              the estimate f^ exactly as nvk_allele_solve_dev defines them: f^ = 0 unless g(0) > 0; f^ = 1 if
 *              g(1) >= 0; otherwise 52 bisection steps on [0, 1] (lo = m when g(m) > 0, else hi = m) and
 *              f^ = (lo + hi) / 2.  L(f^) is evaluated as (the sum of the positive e_i) + (the sum of the logarithms);
 *              exp of a positive number is never formed.
 *   sums       every sum runs over the SITE's rows in row order as 64 interleaved partial sums: row j of the site (not
 *              of the set) goes to sum j mod 64, ascending j; a row outside the set adds +0.0; wave_sum's butterfly adds
 *              the partial sums up.  No atomics: the same bits on every run, and the same bits whether the kernel keeps
 *              a site's rows in registers or reads them again.
 *   outputs    laid out [site][set], every entry written: out_count i64 = the rows of the set, out_fraction f64 = f^,
 *              out_ll f64 = L(f^), 0 where f^ = 0 (and so where the set is empty)
 * All sets of a site are solved in one launch, which is timed under NVK_K_ALLELE.  n_sites == 0 launches nothing (and
 * writes nothing).  0 < clip < inf.  NVK_ERR_INVALID for bad arguments or a NULL array that is not empty (val may be NULL
 * only where n_rows == 0; group may always be).  Device pointers. */
int nvk_mod_site_solve_dev(nvk_ctx *ctx, int64_t n_sites, int64_t n_rows, const int64_t *site_lo, const int64_t *site_hi,
                           const double *val, const int32_t *group, int n_sets, const uint32_t *set_mask, double clip,
                           int64_t *out_count, double *out_fraction, double *out_ll);

/* Model-free per-site summaries (nadavca_amd/site_levels.py: site_levels_batch): the pile-up of the reads' event levels
 * over every reference position and strand.  THE CONTRACT.  The library is built with -ffp-contract=off: every
 * expression below is a rounded operation in the order written.  Inputs are one aligned batch in the flat layout above:
 * signal / sig_off (the windows), events i32[2 total_ref] in slice coordinates as nvk_refine_alignment_batch_dev writes
 * them, expected f64[total_ref] (one level per base, as nvk_expected_signal_batch_dev writes it), per read chunk_start
 * i64 and reverse i32 as nvk_allele_rows_dev uses them, and status (may be NULL: every read counts).
 *   counted base   base g of read j (R = R_j bases, N = N_j samples) with status[j] == 0, trim <= g < R - trim, a
 *                  non-empty event a < b after clamping start and end to 0 .. N (as nvk_event_means_dev does), and a
 *                  global position P = chunk_start[j] + (reverse[j] ? R - 1 - g : g) in [0, ref_len)
 *   key            2 P + (reverse[j] != 0)
 *   values         four doubles, x = the read's window:
 *                    level = np.mean(x[a:b]): numpy's pairwise sum, then one division by n = b - a (the bits of
 *                            nvk_event_means_dev)
 *                    stdv  = np.std(x[a:b]): d = x - level, d * d, numpy's pairwise sum of the squares, / n, sqrt
 *                    dwell = (double)(b - a)
 *                    resid = level - expected[ref_off[j] + g]
 * nvk_site_level_rows_dev writes per base (index ref_off[j] + g): out_key i64[total_ref] (-1 when not counted) and
 * out_val f64[4 total_ref] in the column order above (0.0 four times when not counted).  Events of any length are
 * served.  trim >= 0, 0 <= ref_len <= 2^61; ref_off and sig_off are copied to the host and checked (start at 0, never
 * decrease, ref_off ends at total_ref).
 * nvk_site_moments_dev: key i64[n_rows] is the rows' keys sorted ascending by a STABLE sort (keys < 0 and keys >= n_keys
 * are skipped), val f64[n_rows * n_val] the rows gathered into the same order, 1 <= n_val <= 8.  For every key q in
 * 0 .. n_keys, whose run holds c rows 0 .. c-1 in order, and per column:
 *   S       64 partial sums starting at 0.0, row i added to sum i mod 64 in ascending i, then combined by the butterfly
 *           p[l] = p[l] + p[l xor d] for d = 32, 16, 8, 4, 2, 1 (every lane ends with the same S)
 *   mean    S / c
 *   m2      the same sum of (v - mean) * (v - mean)
 * out_count i64[n_keys] = c, out_mean and out_m2 f64[n_keys * n_val]; mean = m2 = 0.0 where c == 0; every entry of the
 * three is written.  A NaN stays inside its own column.  No atomics: the same bits on every run.
 * NVK_ERR_INVALID for bad arguments or offsets; a data pointer may be NULL only where its array is empty.  Device
 * pointers. */
int nvk_site_level_rows_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                            const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                            const double *expected, const int64_t *chunk_start, const int32_t *reverse,
                            const int32_t *status, int trim, int64_t ref_len, int64_t *out_key, double *out_val);
int nvk_site_moments_dev(nvk_ctx *ctx, int64_t n_rows, int64_t n_keys, int n_val, const int64_t *key, const double *val,
                         int64_t *out_count, double *out_mean, double *out_m2);

/* Per-site rank tests between two samples (nadavca_amd/site_ranks.py: compare_site_ranks, site_rank_tests_batch): the
 * two-sample Kolmogorov-Smirnov and Mann-Whitney statistics of ONE event column over the pile-ups of every listed key,
 * as exact integers, and the exact two-sided p-value of the KS statistic.  THE CONTRACT.  The library is built with
 * -ffp-contract=off: every expression below is a rounded operation in the order written.
 * Inputs, per sample: key i64[n_rows] and val f64[n_rows], the rows of one column sorted ascending by (key, value) (the
 * caller sorts; the order among equal values does not matter; sortedness is the caller's promise and is not checked).
 * Keys are >= 0.  Values hold no NaN; +-inf and -0.0 == 0.0 behave as in C comparisons.  site_key i64[n_sites]: distinct
 * keys, ascending.  Per listed key q, with A the n values of q's run in val_a, B the m values in val_b, and A_lt(x) /
 * A_le(x) (B_lt / B_le) the numbers of A's (B's) values < x / <= x:
 *   n_a, n_b   n and m
 *   ks_plus    the maximum over every x in A u B of A_le(x) m - B_le(x) n: >= 0, and 0 at the largest x; over n m it is
 *              the one-sided statistic D+ of the empirical distribution functions
 *   ks_minus   the same maximum of B_le(x) n - A_le(x) m (D-); the two-sided numerator is h = max(ks_plus, ks_minus)
 *   u2         the sum over x in A of B_lt(x) + B_le(x): twice the Mann-Whitney U of A, ties counting half
 *   tie        the sum over the distinct values of A u B of t^3 - t, t the value's multiplicity in the pooled sample;
 *              this needs n + m < 2^20 per site, which the CALLER guarantees (it is not checked here)
 *   ks_p       the exact two-sided p-value of h under the null hypothesis, ties ignored: the share of the C(n + m, n)
 *              lattice paths from (0, 0) to (n, m) that touch a point with |i m - j n| >= h.  V(i, j) = 1.0 where
 *              |i m - j n| >= h; otherwise V(0, 0) = 0.0 and
 *                V(i, j) = (V(i-1, j) * (double)i + V(i, j-1) * (double)j) / (double)(i + j),
 *              a missing neighbour being 0.0; ks_p = V(n, m).  Computed iff min(n, m) <= 255 and n m <= exact_cells;
 *              NaN otherwise.
 * Where n or m is 0 the four statistics are 0 and ks_p is NaN (n_a and n_b are still the counts).  All outputs i64[n_sites]
 * but out_ks_p f64[n_sites]; every entry of the seven is written.  No atomics and no order-dependent sums: the same bits
 * on every run.  The launch is timed under NVK_K_SITE.  NVK_ERR_INVALID for a negative count, exact_cells < 0, or a NULL
 * pointer where an array is not empty; n_sites == 0 returns NVK_OK.  Device pointers. */
int nvk_site_rank_tests_dev(nvk_ctx *ctx, int64_t n_rows_a, const int64_t *key_a, const double *val_a,
                            int64_t n_rows_b, const int64_t *key_b, const double *val_b, int64_t n_sites,
                            const int64_t *site_key, int64_t exact_cells, int64_t *out_n_a, int64_t *out_n_b,
                            int64_t *out_ks_plus, int64_t *out_ks_minus, int64_t *out_u2, int64_t *out_tie,
                            double *out_ks_p);

/* Per-site two-sample Gaussian mixture tests (nadavca_amd/site_mixtures.py: compare_site_mixtures,
 * site_mixture_tests_batch): per listed key a two-component Gaussian mixture over the pooled values of ONE event column
 * of two samples, the components shared by both: first with one mixing weight (stage 0; the labels are not looked at),
 * then from that solution with one weight per sample (stage 1).  THE CONTRACT.  The library is built with
 * -ffp-contract=off: every expression below is a rounded operation in the order written.
 * Inputs: as nvk_site_rank_tests_dev (rows sorted by (key, value) per sample, site_key distinct and ascending); the
 * values are FINITE (the caller drops the others).  iterations: EM steps per stage, 1 .. 1024; min_sd_ratio in (0, 1].
 * Per listed key q, A the n values of q's run in val_a, B the m values in val_b, N = n + m, fN = (double)N, the pooled
 * rows x_i = A[i] for i < n and B[i - n] beyond.
 *   SUM(f)     64 partial sums starting at 0.0, f(row i) added to sum i mod 64 in ascending i, then combined by the
 *              butterfly p[l] = p[l] + p[l xor d] for d = 32, 16, 8, 4, 2, 1 (nvk_site_moments_dev's sum over the
 *              pooled rows).  Every sum below is one.
 *   one component   mu = SUM(x) / fN; y_i = x_i - mu (every later expression is in y); s = sqrt(SUM(y y) / fN);
 *              ll_one = -fN (log(s) + (C + 0.5)), C = 0.9189385332046727 (log(2 pi) / 2).  c1 = SUM(y > 0 ? 1 : 0),
 *              c0 = fN - c1.  Unless 0 < s < inf, c0 > 0 and c1 > 0 the site is NOT FITTED (see below).
 *              sd_min = min_sd_ratio s.
 *   start      m0 = SUM(y > 0 ? 0 : y) / c0, m1 = SUM(y > 0 ? y : 0) / c1; with d = y - (y > 0 ? m1 : m0):
 *              sd0 = fmax(sqrt(SUM(y > 0 ? 0 : d d) / c0), sd_min), sd1 = fmax(sqrt(SUM(y > 0 ? d d : 0) / c1), sd_min);
 *              wa = wb = c1 / fN.
 *   r(y, w)    i0 = 1 / sd0, i1 = 1 / sd1, ls0 = log(sd0), ls1 = log(sd1); z0 = (y - m0) i0, z1 = (y - m1) i1;
 *              l0 = -0.5 (z0 z0) - ls0, l1 = -0.5 (z1 z1) - ls1; q = l1 - l0; e = exp(-|q|); u = 1 - w;
 *              q > 0: num = w, den = w + u e; otherwise num = w e, den = w e + u; r = num / den where den > 0, else 0
 *              for q > 0 and 1 otherwise.  The row's log density is ld = (q > 0 ? l1 : l0) + log(den) (- C).
 *              A row of A takes w = wa, a row of B w = wb.
 *   EM step    with r_i at the step's parameters: Ra = SUM(i < n ? r : 0), Rb = SUM(i < n ? 0 : r), R0 = SUM(1 - r),
 *              T1 = SUM(r y), T0 = SUM((1 - r) y); R1 = Ra + Rb.  Unless R1 > 0 and R0 > 0 the stage ENDS here, the
 *              parameters unchanged.  Otherwise m0' = T0 / R0, m1' = T1 / R1, with the SAME r_i
 *              sd0' = fmax(sqrt(SUM((1 - r) ((y - m0') (y - m0'))) / R0), sd_min) and sd1' likewise from r, m1', R1;
 *              stage 0: wa' = wb' = R1 / fN; stage 1: wa' = Ra / (double)n, wb' = Rb / (double)m.
 *   a stage    up to `iterations` EM steps, then at its final parameters ll = SUM(ld) - fN C, and in stage 0 also
 *              Ra, Rb as above, rbar = (Ra + Rb) / fN and Q = SUM((r - rbar) (r - rbar)).  Stage 1 starts from stage
 *              0's final parameters.
 * out_counts i64[5 n_sites], per site: n, m, fitted (0 / 1), the EM steps run in stage 0 and in stage 1.
 * out_fit f64[17 n_sites], per site: ll_one | stage 0: mu + m0, sd0, mu + m1, sd1, w, ll_shared, Ra, Rb, Q | stage 1:
 * mu + m0, sd0, mu + m1, sd1, wa, wb, ll_free.  A site that is not fitted has fitted = 0, no steps, ll_shared = ll_free
 * = ll_one (+inf where every value is the same) and NaN in the other fourteen; where n or m is 0 all seventeen are NaN.
 * Every entry is written.  Sites of up to 128 rows keep y and r in registers, larger ones recompute them: the same
 * expressions and the same bits.  No atomics: the same bits on every run.  The launch is timed under NVK_K_SITE.
 * NVK_ERR_INVALID for a negative count, iterations or min_sd_ratio outside their ranges, or a NULL pointer where an
 * array is not empty; n_sites == 0 returns NVK_OK and writes nothing.  Device pointers. */
int nvk_site_mixture_tests_dev(nvk_ctx *ctx, int64_t n_rows_a, const int64_t *key_a, const double *val_a,
                               int64_t n_rows_b, const int64_t *key_b, const double *val_b, int64_t n_sites,
                               const int64_t *site_key, int iterations, double min_sd_ratio, int64_t *out_counts,
                               double *out_fit);

/* The base -> sample table of a read from its signal and its sequence alone (nadavca_amd/signal_map.py:
 * signal_map_batch): event detection, then an adaptive-banded alignment of the events to the k-mer levels of the read's
 * own bases, as nanopolish / f5c eventalign and tombo resquiggle rebuild it.  THE CONTRACT.  The library is built with
 * -ffp-contract=off: every expression below is a rounded f64 operation in the order written; a sum over a range is an
 * ascending loop from 0.  The CPU restatements the tests hold the kernels to bit for bit are
 * tests/host_shims/events_host.cpp and eventalign_host.cpp.
 *
 * EVENT DETECTION.  Read j's samples are x = signal[sig_off[j] .. sig_off[j+1]) (n samples, normalised by the caller),
 * w = window (1..8), fw = (double)w.
 *   statistic   for w <= i <= n - w, over L = x[i-w .. i) and R = x[i .. i+w):
 *                 mL = SUM(L) / fw, vL = SUM((x - mL) (x - mL)) / fw, mR and vR alike, d = mR - mL,
 *                 s(i) = (fw * (d * d)) / ((vL + vR) + var_floor);   s(i) = 0 for every other i
 *   border      sample i, 0 <= i < n, when i == 0, or s(i) >= threshold and s(i) > s(u) for i - w < u < i and
 *               s(i) >= s(u) for i < u < i + w (the first of equal values wins).  threshold > 0, var_floor > 0.
 *   event       from a border to the next border of the read or to the read's end: no event crosses two reads
 * nvk_event_flags_dev writes out_flags i32[total_signal]: 1 at a border, else 0.  The caller lists the flat positions
 * of the borders in ascending order (ev_pos i64[n_events]; the per-read counts are a prefix sum over the flags) and
 * nvk_event_levels_dev writes per event e, with a = ev_pos[e], in the read that owns sample a, and b = the smaller of
 * ev_pos[e+1] (total_signal for the last event) and that read's end: out_start = a - sig_off[read] (i32), out_len =
 * b - a (i32), out_level = SUM(signal[a .. b)) / (double)(b - a).  sig_off is copied to the host and checked (starts
 * at 0, never decreases, ends at total_signal, no read above 2^31 - 1 samples).  NVK_ERR_INVALID for bad arguments,
 * NVK_ERR_UNSUPPORTED for window > 8.  Device pointers. */
int nvk_event_flags_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_signal, const double *signal,
                        const int64_t *sig_off, int window, double threshold, double var_floor, int32_t *out_flags);
int nvk_event_levels_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_signal, const double *signal,
                         const int64_t *sig_off, int64_t n_events, const int64_t *ev_pos, int32_t *out_start,
                         int32_t *out_len, double *out_level);

/* EVENT ALIGNMENT.  Read j has E events with levels e_i = level[ev_off[j] + i] and K bases with, per base,
 * mu / ac / mc [base_off[j] + b]: the level of the base's k-mer and the constants of its Gaussian, ac = -log(sd sqrt(2
 * pi)), mc = 1 / (2 sd sd), computed by the caller; l_stay[j] and l_step[j] are the read's transition costs (logs,
 * computed by the caller); trim_cost and skip_cost are finite and <= 0.  NINF = -infinity.  The kernel only adds,
 * multiplies and compares.
 *   cells      (i, b), 0 <= i < E, 0 <= b < K;  em(i, b) = ac[b] - ((e_i - mu[b]) * (e_i - mu[b])) * mc[b]
 *   step       = (src + l_step) + em, src = S(i-1, b-1) for b > 0, and for b == 0 the free start (double)i * trim_cost
 *   stay       = (S(i-1, b) + l_stay) + em
 *   skip       = S(i, b-1) + skip_cost for b > 0, NINF for b == 0 (no emission)
 *   S(i, b)    the largest of the three, the first of equal ones in the order step, stay, skip; a neighbour outside
 *              the matrix or outside its band is NINF
 *   bands      E + K + 1 anti-diagonal bands of `band` cells (64 or 128), H = band / 2.  Band t has a corner (et, kt);
 *              its cell at offset o, 0 <= o < band, is (et - o, kt + o), so band t holds cells with i + b = t - 2.
 *              Band 0: (H - 1, -1 - H); band 1 moves down.  Band t >= 2 moves right (kt = k(t-1) + 1) when ll < ur and
 *              down (et = e(t-1) + 1) otherwise, ll and ur being the values of band t-1 at offsets 0 and band - 1; when
 *              both are NINF it moves right for odd t.  For this purpose alone a position (i, -1), -1 <= i < E, has
 *              the value (double)(i + 1) * trim_cost (the trimmed column: it holds the band on the events a free start
 *              trims and feeds no cell); every other position outside the matrix has NINF.
 *   end        the cell (i, K-1) inside its band with the largest S(i, K-1) + (double)(E - 1 - i) * trim_cost, the
 *              smallest i among equal ones; that sum is out_score
 *   walk back  from the end: a skip leaves the base; a stay goes to (i-1, b); a step goes to (i-1, b-1), or ends the
 *              walk at b == 0 (first_event = i).  A base's first event is the smallest i of its cells that the walk
 *              leaves by step or stay; a base the walk only skips through has none (-1).
 *   status     0 mapped; NVK_MAP_NO_EVENTS: E == 0 or K == 0; NVK_MAP_LOST: no cell of column K-1 lies in a band or
 *              all of them are NINF, the walk leaves the bands, or more than an eighth of the bases have no event
 *              (8 * skipped > K: the path no longer follows the signal).  status_in (i32 per read, may be NULL): a read
 *              with a non-zero entry is not aligned and reports that entry.
 * out_hit i32[4 n_reads]: per read (status, E, first_event, last_event); out_score f64[n_reads]; out_base_event
 * i32[total_bases]: per base its first event, counted inside the read, or -1.  A read with non-zero status has -1 in
 * every base, first_event = last_event = -1 and out_score = NINF.
 * The traceback store takes band / 4 bytes per band (2 bits per cell, band-major) and one bit per band for its move;
 * its size is bounded by nvk_ctx_set_workspace_limit's cap: when a batch's store is larger its reads run in parts that
 * fit (a single read larger than the cap runs on its own); results do not change.  ev_off and base_off are copied to
 * the host and checked (start at 0, never decrease, end at total_events / total_bases, no read above 2^26 events or
 * bases).  NVK_ERR_INVALID for bad arguments, NVK_ERR_UNSUPPORTED for a band other than 64 or 128.  Device pointers. */
enum { NVK_MAP_OK = 0, NVK_MAP_NO_EVENTS = 1, NVK_MAP_LOST = 2 };
int nvk_event_align_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                        const int64_t *ev_off, int64_t total_bases, const double *mu, const double *ac,
                        const double *mc, const int64_t *base_off, const double *l_stay, const double *l_step,
                        const int32_t *status_in, int band, double trim_cost, double skip_cost, int32_t *out_hit,
                        double *out_score, int32_t *out_base_event);

/* SIGNAL LOCATION (signal_locate_batch).  A subsequence alignment of every query against every column of every target:
 * query q has Q events with levels e_i = level[q_off[q] + i], already rescaled by the caller, 0 <= Q <= max_events <=
 * 256; target t has L columns with, per column, mu / ac / mc [col_off[t] + j] (as for the event alignment above).
 * l_stay, l_step, l_skip and trim_cost are finite and <= 0.  NINF = -infinity.  Every expression is a rounded f64
 * operation in the order written; the kernel only adds, multiplies and compares.
 *   cells      (i, j), 0 <= i < Q, 0 <= j < L;  em(i, j) = ac[j] - ((e_i - mu[j]) * (e_i - mu[j])) * mc[j]
 *   candidates open = (double)i * trim_cost          the path starts here, events 0 .. i-1 trimmed
 *              step = S(i-1, j-1) + l_step
 *              stay = S(i-1, j) + l_stay
 *              skip = S(i-1, j-2) + l_skip
 *              a neighbour outside the target, or with i == 0, is NINF: nothing crosses from one target to the next
 *   S(i, j)    = v + em(i, j), v the largest candidate, the first of equal ones in the order open, step, stay, skip.
 *              A cell carries (start column, first event): its own (j, i) when open wins, else its source's.
 *   end        end(i, j) = S(i, j) + (double)(Q - 1 - i) * trim_cost; a column's best is its largest end value, the
 *              smallest i among equal ones (a column without an end value above NINF has none)
 *   blocks     target t is cut into blocks of NVK_LOC_BLOCK = 256 columns, the last one short; blocks are numbered over
 *              all targets in order, n_blocks = SUM ceil(L / 256).  A block's best is the largest best of its columns,
 *              the smallest column among equal ones.
 * Every move consumes one event, so S(i, j) depends on the columns [j - 2 i, j] alone and a target may be swept as
 * independent tiles that overlap by 2 (max_events - 1) columns: the results do not depend on the cut, nor on
 * max_events beyond that it bounds Q.
 * out_score f64[n_queries * n_blocks]: the block's best end value, query-major; out_hit i32[4 * n_queries * n_blocks]:
 * (end column inside the target, last event i, start column inside the target, first event).  A block without a best
 * (Q == 0) has NINF and -1 four times.  q_off and col_off are copied to the host and checked (start at 0, never
 * decrease, end at total_events / total_cols, no query above max_events events, no target above 2^30 columns);
 * n_blocks must be the count above.  NVK_ERR_INVALID for bad arguments, NVK_ERR_UNSUPPORTED for max_events > 256;
 * NVK_OK with nothing written for n_queries == 0 or n_targets == 0.  Device pointers. */
enum { NVK_LOC_OK = 0, NVK_LOC_NO_EVENTS = 1, NVK_LOC_AMBIGUOUS = 2 };   /* per-read status of signal_locate_batch */
enum { NVK_LOC_BLOCK = 256, NVK_LOC_MAX_EVENTS = 256 };
int nvk_signal_locate_dev(nvk_ctx *ctx, int64_t n_queries, int64_t total_events, const double *level,
                          const int64_t *q_off, int64_t n_targets, int64_t total_cols, const double *mu,
                          const double *ac, const double *mc, const int64_t *col_off, int max_events, double l_stay,
                          double l_step, double l_skip, double trim_cost, int64_t n_blocks, double *out_score,
                          int32_t *out_hit);

/* VITERBI DECODE (decode_batch).  The classic k-mer HMM decode: per read the best path of its events over the 4^k
 * k-mer states, the base sequence the path spells and, per base, the first event of the state that owns it (the move
 * table).  Read r has E events with levels e_i = level[ev_off[r] + i], already rescaled by the caller and finite; the
 * table is mean / ac / mc f64[4^k], ac = -log(sd sqrt(2 pi)), mc = 1 / (2 sd sd), computed by the caller; k in 2..6,
 * alphabet 4, central in 0..k-1; l_stay, l_step and l_skip are finite and <= 0.  NINF = -infinity.  Every expression is
 * a rounded f64 operation in the order written; the kernel only adds, multiplies and compares.
 *   states     a state is a k-mer id as csrc/kmer.h numbers it, the first base most significant; S = 4^k,
 *              0 <= s < S; `div` and `mod` are those of non-negative integers
 *   em(i, s)   = ac[s] - ((e_i - mean[s]) * (e_i - mean[s])) * mc[s]
 *   V(0, s)    = em(0, s)
 *   i >= 1     with P = V(i-1, .):
 *              step: a* = the smallest a in 0..3 with the largest P[a * 4^(k-1) + s div 4]; that value + l_step
 *              stay: P[s] + l_stay
 *              skip: c* = the smallest c in 0..15 with the largest P[c * 4^(k-2) + s div 16]; that value + l_skip
 *              V(i, s) = v + em(i, s), v the largest candidate, the first of equal ones in the order step, stay, skip.
 *              The arg-maxima are taken on P, before the cost is added.
 *   end        the smallest s with the largest V(E-1, s); that value is out_score
 *   walk back  from (E-1, end state): a stay goes to (i-1, s), a step to (i-1, a* 4^(k-1) + s div 4), a skip to
 *              (i-1, c* 4^(k-2) + s div 16)
 *   sequence   the k letters of the state at event 0, the first base first; then, event after event, one letter per
 *              step (s mod 4 of the state entered) and two per skip ((s div 4) mod 4, then s mod 4):
 *              n_bases = k + steps + 2 skips
 *   owner      the state at event 0 owns base `central`; a step moves the owner on by one, a skip by two.
 *              out_base_event[b] = the smallest event at which the path is in the state that owns b; -1 for the base a
 *              skip passes, for the first `central` bases and for the last k - 1 - central.
 *   status     NVK_DEC_OK; NVK_DEC_NO_EVENTS: E == 0; status_in (i32 per read, may be NULL): a read with a non-zero
 *              entry is not decoded and reports that entry.  A read that is not decoded has n_bases 0, end state -1 and
 *              out_score NINF.
 * out_hit i32[4 n_reads]: per read (status, E, n_bases, end state); out_score f64[n_reads]; out_seq and out_base_event
 * i32[total_cap]: read r's n_bases entries from cap_off[r] on (what lies between them and cap_off[r+1] is scratch).
 * cap_off[r+1] - cap_off[r] >= k + 2 (E - 1) for every read with E >= 1.
 * The traceback store takes 4^k / 2 bytes per event but a read's first (per 16 states one 8-byte word: c*, four a* and
 * sixteen 2-bit choices); its size is bounded by nvk_ctx_set_workspace_limit's cap, and by 4 GiB or 60 % of the free
 * device memory, whichever is less, on a context without a limit (4 GiB: 2 566 reads of 818 events at k = 6).  When a
 * batch's store is larger its reads run in parts that fit (a single read larger than the cap runs on its own); results
 * do not change.  The store's workspace stays reserved, up to that cap, until the context is destroyed.  out_parts
 * (host pointer, may be NULL): the number of parts the batch ran in.  ev_off and cap_off are
 * copied to the host and checked (start at 0, never decrease, end at total_events / total_cap, no read above 2^26
 * events, the capacities above).  NVK_ERR_UNSUPPORTED for k outside 2..6, NVK_ERR_INVALID for other bad arguments;
 * NVK_OK with nothing written for n_reads == 0.  Device pointers but out_parts. */
enum { NVK_DEC_OK = 0, NVK_DEC_NO_EVENTS = 1 };   /* per-read status of decode_batch */
int nvk_viterbi_decode_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                           const int64_t *ev_off, int k, int central, const double *mean, const double *ac,
                           const double *mc, double l_stay, double l_step, double l_skip, const int32_t *status_in,
                           int64_t total_cap, const int64_t *cap_off, int32_t *out_hit, double *out_score,
                           int32_t *out_seq, int32_t *out_base_event, int64_t *out_parts);

/* K-MER POSTERIORS (decode_batch(qualities=True)).  The forward-backward recurrences over the same 4^k states and the
 * same three moves as the Viterbi decode above, with sums where that one takes maxima: per event the posterior of each
 * of the four letters at position `pos` of the state (first base = 0; pos in 0..k-1), and per read the likelihood of
 * its events summed over all paths.  level / ev_off, k, mean / ac / mc, status_in and em(i, s) are the Viterbi
 * contract's.  w_stay, w_step and w_skip are the moves' linear weights, each finite and in (0, 1], with
 * max(w_stay, w_step) >= 2^-10 (the caller passes the numbers whose logs the Viterbi call takes).  Every expression is
 * a rounded f64 operation in the order written (-ffp-contract=off); fma is the fused operation; the kernels call no
 * library exp or log.  Q = 4^(k-1), T = 4^(k-2), S = 4^k.
 *   EXP(g)     y = g * LOG2E (0x1.71547652b82fep+0), n = rint(y), EXP = ldexp(P(y - n), (int)n); P is the fma chain of
 *              xm::exp2_frac_horner (csrc/xmath.h): p = c11; p = fma(p, f, c10); ...; P = fma(p, f, 1.0)
 *   b(i, s)    = EXP(max(em(i, s), -300.0)).  With the floor a row's largest value, and the product of a forward and a
 *              backward value at the best state, stay normal doubles; an event far from every state becomes
 *              uninformative instead of zeroing the row
 *   frexp      "the exponent of v": the x with v = m * 2^x, m in [0.5, 1)
 *   forward    A(0, s) = b(0, s), X_0 = 0.  For i >= 1, with P = A(i-1, .): x = the exponent of max_s P[s];
 *              sum4  = ((P[0 Q + q] + P[1 Q + q]) + P[2 Q + q]) + P[3 Q + q], q = s div 4;
 *              sum16 = the same over c = 0..15 ascending, of P[c T + s div 16];
 *              t = ((w_step * sum4) + (w_stay * P[s])) + (w_skip * sum16);
 *              A(i, s) = ldexp(t, -x) * b(i, s);  X_i = X_(i-1) + x
 *   backward   B(E-1, s) = 1.  For i = E-2 down to 0: W[s'] = B(i+1, s') * b(i+1, s');
 *              G4[r] = ((W[4r] + W[4r+1]) + W[4r+2]) + W[4r+3] for r < Q;
 *              G16[r] = ((G4[4r] + G4[4r+1]) + G4[4r+2]) + G4[4r+3] for r < T;  y = the exponent of max_s B(i+1, s);
 *              B(i, s) = ldexp(((w_step * G4[s mod Q]) + (w_stay * W[s])) + (w_skip * G16[s mod T]), -y)
 *              (the successors of s are the states whose Viterbi predecessor is s: by a step (s mod Q) 4 + 0..3, by a
 *              skip (s mod T) 16 + 0..15)
 *   sums over  (Z and the class sums) within a block of 16 consecutive states ascending, a block without a term giving
 *   all states 0; over the T blocks v[u] the butterfly of wave_sum: for d = min(T, 64) / 2, ..., 1: v[u] = v[u] + v[u xor d]
 *              for every u at once; for T = 256 the four groups of 64 blocks then join as (g0 + g1) + (g2 + g3)
 *   outputs    C_x(i) = the sum of A(i, s) * B(i, s) over the states whose letter at pos is x;
 *              out_marg[4 (ev_off[r] + i) + x] = C_x / (((C_0 + C_1) + C_2) + C_3): self-normalised, no exponent enters.
 *              out_z[2 r] = the sum of A(E-1, .), out_z[2 r + 1] = (double)X_(E-1): log Z = log(out_z[2 r]) +
 *              out_z[2 r + 1] ln 2 is left to the caller.
 *              out_status[r] = NVK_DEC_OK; NVK_DEC_NO_EVENTS: E == 0; else the read's non-zero status_in entry.  A read
 *              that is not processed writes no marginals and reports out_z = (0, 0).
 * out_marg f64[4 total_events], out_z f64[2 n_reads], out_status i32[n_reads].
 * The forward sweep keeps every A(i, .) in a row store of 8 * 4^k bytes per event, which the backward sweep, a second
 * launch, reads back.  The store's size is bounded by nvk_ctx_set_workspace_limit's cap, and by 16 GiB or 60 % of the
 * free device memory, whichever is less, on a context without a limit (at k = 6 a read of 816 events takes 26.7 MB:
 * 4 GiB would hold 160 such reads, fewer workgroups than the device has CUs; 16 GiB holds 640).  When a batch's store
 * is larger its reads run in parts that fit, the forward and the backward sweep of a part before the next part's (a
 * single read larger than the cap runs on its own); results do not change.  The store shares the Viterbi store's
 * workspace, which stays reserved, up to that cap, until the context is destroyed.  out_parts (host pointer, may be
 * NULL): the number of parts.  out_ms (host pointer to two doubles, may be NULL): the milliseconds of the forward and of
 * the backward launches, summed over the parts, by HIP events; with it the call waits for every part before it starts
 * the next.  ev_off is copied to the host and checked (starts at 0, never decreases, ends at total_events, no read
 * above 2^26 events).  NVK_ERR_UNSUPPORTED for k outside 2..6, NVK_ERR_INVALID for other bad arguments; NVK_OK with
 * nothing written for n_reads == 0.  Device pointers but out_parts and out_ms. */
int nvk_kmer_posterior_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                           const int64_t *ev_off, int k, int pos, const double *mean, const double *ac,
                           const double *mc, double w_stay, double w_step, double w_skip, const int32_t *status_in,
                           double *out_marg, double *out_z, int32_t *out_status, int64_t *out_parts, double *out_ms);

/* K-MER EXPECTATIONS (decode_batch(fit=n)).  The E-step of a Baum-Welch fit over the same states, moves and sweeps as
 * the posteriors above: per read the expected number of each move and the posterior-weighted moments of its events'
 * levels against the states' means.  The inputs are nvk_kmer_posterior_dev's without `pos`; EXP, b, frexp, forward (A,
 * X), backward (B, W, G4, G16) and the rule for sums over all states are that contract's, and the forward sweep is its
 * own kernel, so out_z's bits are that call's.  Every expression is a rounded f64 operation in the order written; the
 * kernels call no library exp or log and use no atomics.  x_i = level[ev_off[r] + i].
 *   per event  i = E-1 down to 0, every sum over all states by the rule above:
 *              D  = sum of A(i, s) * B(i, s)
 *              m0 = sum of (A(i, s) * B(i, s)) * mc[s];  m1 = sum of ((A * B) * mc[s]) * mean[s];
 *              m2 = sum of (((A * B) * mc[s]) * mean[s]) * mean[s]
 *              M0 += m0 / D;  Mx += (m0 / D) * x_i;  Mxx += ((m0 / D) * x_i) * x_i;
 *              Mm += m1 / D;  Mxm += (m1 / D) * x_i;  Mmm += m2 / D
 *              F += 1.0 when the largest em(i, s) over s is <= -300.0 (every b(i, .) sits on the floor: the event's
 *              Gaussian moments are the floor's, not the model's)
 *   per move   i -> i + 1, for i < E-1, with W, G4 and G16 those the backward recurrence forms from event i + 1:
 *              n_stay = sum of A(i, s) * (w_stay * W[s]);  n_step = sum of A(i, s) * (w_step * G4[s mod Q]);
 *              n_skip = sum of A(i, s) * (w_skip * G16[s mod T]);  t = (n_stay + n_step) + n_skip;
 *              N_stay += n_stay / t;  N_step += n_step / t;  N_skip += n_skip / t
 *              (ratios inside one event: no exponent enters; the three shares of a move sum to 1, so the three N sum
 *              to E - 1 up to rounding)
 *   order      every accumulator starts at 0.0 and takes its terms with i descending
 * out_stats f64[10 n_reads]: per read (M0, Mx, Mxx, Mm, Mxm, Mmm, N_stay, N_step, N_skip, F).  out_z, out_status,
 * out_parts and out_ms ([0] the forward launches, [1] the counts launches) are nvk_kmer_posterior_dev's; a read that is
 * not processed writes no stats and reports out_z = (0, 0).  The row store, its cap, the cut into parts (results do not
 * change), the checks and the return codes are that call's.  Device pointers but out_parts and out_ms. */
int nvk_kmer_expectations_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                              const int64_t *ev_off, int k, const double *mean, const double *ac, const double *mc,
                              double w_stay, double w_step, double w_skip, const int32_t *status_in,
                              double *out_stats, double *out_z, int32_t *out_status, int64_t *out_parts,
                              double *out_ms);

/* K-MER STATE MOMENTS (estimate_decode_model).  The part of Baum-Welch that adapts the table: per state the posterior
 * weight of the batch's events and the first two moments of their levels under it.  The inputs are
 * nvk_kmer_expectations_dev's; EXP, b, frexp, forward (A, X), backward (B, W, G4, G16) and the rule for sums over all
 * states are that contract's, and the forward sweep is the same kernel, so out_z's bits are nvk_kmer_posterior_dev's.
 * Every expression is a rounded f64 operation in the order written; the kernels call no library exp or log and use no
 * atomics.  x_i = level[ev_off[r] + i], S = 4^k.
 *   per event   i = E-1 down to 0:
 *               D   = sum over all states of A(i,s) * B(i,s)          (the expectations contract's D, same bits)
 *               inv = 1.0 / D
 *               g   = (A(i,s) * B(i,s)) * inv
 *               G0[s] = G0[s] + g;   G1[s] = G1[s] + g * x_i;   G2[s] = G2[s] + (g * x_i) * x_i
 *               every accumulator starts at 0.0 and takes its terms with i descending
 *   per batch   tot[m][s] starts at 0.0 and takes the reads with status NVK_DEC_OK in ascending read order:
 *               tot[m][s] = tot[m][s] + G_m[s] of the read.  A read that is not processed adds nothing.
 * out_moments f64[3 * 4^k], laid out [m][s]; out_z, out_status, out_parts as nvk_kmer_posterior_dev;
 * out_ms (may be NULL): three doubles, the forward, the moments and the reduce launches summed over the parts.
 * The moments sweep leaves every read's 3 S sums in a slab of a workspace of its own (the part's reads times 24 * 4^k
 * bytes) and a third launch chains the part's slabs, in read order, onto the totals the parts before it left; the
 * totals are zeroed on the stream when the call starts.  So the result does not depend on the cut into parts.  A read
 * counts in the cut with its rows and its slab (its events and three rows more), so that rows plus slabs stay under
 * the row store's cap; the store, the cap, the checks and the return codes are nvk_kmer_posterior_dev's (NVK_OK with
 * nothing written for n_reads == 0).  Device pointers but out_parts and out_ms. */
int nvk_kmer_state_moments_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                               const int64_t *ev_off, int k, const double *mean, const double *ac, const double *mc,
                               double w_stay, double w_step, double w_skip, const int32_t *status_in,
                               double *out_moments, double *out_z, int32_t *out_status, int64_t *out_parts,
                               double *out_ms);

/* REPEAT COUNT (count_repeats_batch).  The best path of an item's events over a short chain of k-mer states with one
 * back edge, the loop of a tandem repeat: how often the path goes round the loop is the repeat's copy number less the
 * copies the chain spells out.  Chain c has N = st_off[c+1] - st_off[c] states, 3 <= N <= NVK_REP_MAX_STATES = 256,
 * with, per state, mu / ac / mc [st_off[c] + j] (as for the event alignment above), and four integers chain_par[4 c ..
 * 4 c + 3] = (lp_from, lp_to, m1, m2) with 0 <= lp_to < lp_from < m2 <= N - 1 and 1 <= m1 <= m2: the back edge goes
 * from state lp_from to state lp_to; m1 and m2 are marks (for a repeat: its first state and the first state after it).
 * Item t is items[3 t .. 3 t + 2] = (chain, ev_lo, ev_hi): the E = ev_hi - ev_lo events e_i = level[ev_lo + i],
 * already rescaled by the caller; items may share events (the usual pair: the two strands of one read).  l_stay,
 * l_step, l_skip and trim_cost are finite and <= 0.  NINF = -infinity.  Every expression is a rounded f64 operation in
 * the order written; the kernel only adds, multiplies and compares.
 *   cells      (i, j), 0 <= i < E, 0 <= j < N;  em(i, j) = ac[j] - ((e_i - mu[j]) * (e_i - mu[j])) * mc[j]
 *   candidates open = (double)i * trim_cost          j == 0 only: the path starts here, events 0 .. i-1 trimmed
 *              step = S(i-1, j-1) + l_step
 *              loop = S(i-1, lp_from) + l_step       j == lp_to only: the back edge is taken by a step, never a skip
 *              stay = S(i-1, j) + l_stay
 *              skip = S(i-1, j-2) + l_skip
 *              a source outside the chain, or with i == 0, is NINF
 *   S(i, j)    = v + em(i, j), v the largest candidate, the first of equal ones in the order open, step, loop, stay,
 *              skip.  A cell without a candidate above NINF is NINF; it carries nothing and feeds no cell that counts.
 *   carried    instead of a traceback, by every cell from the source of its winning candidate:
 *              loops   the source's, + 1 when loop wins; 0 when open wins
 *              first   the source's; i when open wins
 *              marks   for q = 1, 2 the pair (v_q, i_q): the source's; (v, i) when j >= m_q and the winning source state
 *                      is below m_q (open counts as state -1): the candidate value and the event with which the path
 *                      enters the states from m_q on.  Unset: (NINF, -1).  The loop's source lies below m2 and its
 *                      target below it, so going round the loop sets no mark anew.
 *   end        end(i) = S(i, N-1) + (double)(E - 1 - i) * trim_cost; the result is the largest end value, the smallest
 *              i among equal ones: `last`
 *   status     NVK_REP_OK; NVK_REP_NO_EVENTS: E == 0; NVK_REP_NO_PATH: no end value above NINF (fewer events than the
 *              shortest way through the chain); status_in (i32 per item, may be NULL): an item with a non-zero entry
 *              is not run and reports that entry.
 * out_hit i32[8 n_items]: per item (status, E, first, last, loops, i1, i2, 0), the carried values of (last, N-1);
 * out_score f64[4 n_items]: (end(last), S(last, N-1), v1, v2).  An item that is not NVK_REP_OK has -1 in first, last,
 * loops, i1 and i2 and NINF in its four scores.  v1 - first * trim_cost is what the path scored before the first mark,
 * v2 - v1 between the marks, S(last, N-1) - v2 from the second mark on.
 * One wave per item, the chain's tables and the row in registers: no workspace.  st_off, chain_par and items are copied
 * to the host and checked (the offsets start at 0, never decrease and end at total_states; the chain integers as above;
 * every item's chain below n_chains and 0 <= ev_lo <= ev_hi <= total_events, no item above 2^26 events).
 * NVK_ERR_UNSUPPORTED for a chain above 256 states, NVK_ERR_INVALID for other bad arguments; NVK_OK with nothing
 * written for n_items == 0.  out_ms (host pointer to one double, may be NULL): the milliseconds of the launches, by HIP
 * events.  Device pointers but out_ms; out_hit and out_score aligned to 16 bytes. */
enum { NVK_REP_OK = 0, NVK_REP_NO_EVENTS = 1, NVK_REP_NO_PATH = 2 };   /* per-item status of count_repeats_batch */
enum { NVK_REP_MAX_STATES = 256 };
int nvk_repeat_count_dev(nvk_ctx *ctx, int64_t n_items, const int64_t *items, int64_t total_events,
                         const double *level, int64_t n_chains, int64_t total_states, const double *mu,
                         const double *ac, const double *mc, const int64_t *st_off, const int32_t *chain_par,
                         double l_stay, double l_step, double l_skip, double trim_cost, const int32_t *status_in,
                         int32_t *out_hit, double *out_score, double *out_ms);

/* REPEAT LIKELIHOODS (count_repeats_batch(layers=n)).  Beside the best path of REPEAT COUNT, the sum over all paths: for
 * every c in 0 .. L-1 the likelihood of an item's events summed over the paths that go round the chain's loop exactly
 * c times.  items, level, the chains (mu / ac / mc, st_off, chain_par), status_in and em(i, j) are the REPEAT COUNT
 * contract's, with its checks of chains and items; the marks m1 and m2 are checked and not used.  w_stay, w_step,
 * w_skip and w_trim are the moves' and the trim's linear weights, each finite and in (0, 1], with max(w_stay, w_step)
 * >= 2^-10 (the caller passes the numbers whose logs the Viterbi call takes).  layers = L, 1 <= L <=
 * NVK_REP_MAX_LAYERS = 128.  EXP, the floor b(i, j) = EXP(max(em(i, j), -300.0)) and "the exponent of v" are the K-MER
 * POSTERIORS contract's.  Every expression is a rounded f64 operation in the order written (-ffp-contract=off); no
 * library exp or log.
 *   trellis    (i, c, j): event i, layer c = the trips round the loop so far, chain state j.  Values are kept scaled:
 *              A^(i, ., .) = A(i, ., .) * 2^(-X_i).  z_c is the scaled sum over the paths of layer c that have ended
 *              in state N-1, the events after their last one trimmed at w_trim each; o_i the scaled weight w_trim^i
 *              of opening at event i.
 *   row 0      A^(0, 0, 0) = b(0, 0), every other cell +0.0; o_0 = 1.0, X_0 = 0, z_c = A^(0, c, N-1)
 *   row i >= 1 with P = A^(i-1, ., .):
 *              x = the exponent of the largest of P over all layers and states and of z_c over all layers (0 when
 *                  all of them are 0)
 *              o_i = ldexp(o_(i-1) * w_trim, -x)
 *              t = (((w_step * P[c][j-1]) + (w_step * P[c-1][lp_from])) + (w_stay * P[c][j])) + (w_skip * P[c][j-2]);
 *                  the second term counts only at j == lp_to and c >= 1: the back edge is taken by a step only; a term
 *                  that does not exist (a source outside the chain, no loop term, layer -1) is +0.0
 *              A^(i, c, j) = (ldexp(t, -x) + q) * b(i, j), q = o_i at (c, j) = (0, 0) and +0.0 elsewhere
 *              z_c = ldexp(z_c * w_trim, -x) + A^(i, c, N-1);  X_i = X_(i-1) + x
 *              A path that would need layer L is dropped, not pooled into the last layer.
 *   outputs    out_z f64[n_items * L]: item t's z_c after the last event at [t L + c]; out_x f64[n_items]:
 *              (double)X_(E-1); log L(loops = c) = log(out_z) + out_x ln 2 is left to the caller.
 *              out_status i32[n_items]: NVK_REP_OK; NVK_REP_NO_EVENTS: E == 0; NVK_REP_NO_PATH: every z_c is 0; else the
 *              item's non-zero status_in entry.  An item that is not run (no events, a status_in entry) writes zeros
 *              to out_z and out_x.
 * THE SCALE.  The z_c take part in x because they, unlike the cells, do not shrink with the emissions: a path that
 * has ended pays w_trim per later event where a live one pays about w * b, and after three events whose every
 * emission sits on the floor a z_c scaled by the cells alone would be e^900 w_trim^3 times the largest cell, above
 * the largest double.  With x as above every scaled value of row i-1 is below 1 after the ldexp, a row's sum has at
 * most four terms of weight <= 1, and b <= EXP(max ac): nothing overflows; nor does o_i, which is at most e^300 times
 * the largest cell of its row because A^(i, 0, 0) >= o_i b(i, 0).  What can happen is
 * underflow, and it is harmless: a value vanishes only when it is 2^-1022 of the largest, in a likelihood that holds
 * the largest as a term.  That largest value M of a row is a positive normal double whenever the row before it had
 * one and w_stay >= 2^-10: a stay keeps the cell that held it, M_i >= w_stay b M_(i-1) >= 2^-10 e^-300 / 2, and a z_c
 * stays through w_trim alone (a w_trim below 2^-1021 can flush it).  With w_stay < 2^-10 <= w_step the same holds for
 * every cell but those of state N-1, which alone has no step out: a row whose weight sits in that state alone, with a
 * w_stay below 2^-588, can vanish; x is then 0, the z_c keep what had ended, and the call reports what is left
 * (NVK_REP_NO_PATH when nothing is).  Row 0 has b(0, 0) >= e^-300.
 * One workgroup per item, ceil(L / LB) waves of 64 with LB = 32 layers per wave for chains of up to 64 states and 16
 * above; rows in registers, no workspace, no atomics.  No sum crosses lanes: the result does not depend on an order of
 * lanes or waves.  NVK_ERR_UNSUPPORTED for L above 128 or a chain above 256 states, NVK_ERR_INVALID for other bad
 * arguments; NVK_OK with nothing written for n_items == 0.  out_ms as in nvk_repeat_count_dev.  Device pointers but
 * out_ms. */
enum { NVK_REP_MAX_LAYERS = 128 };
int nvk_repeat_likelihoods_dev(nvk_ctx *ctx, int64_t n_items, const int64_t *items, int64_t total_events,
                               const double *level, int64_t n_chains, int64_t total_states, const double *mu,
                               const double *ac, const double *mc, const int64_t *st_off, const int32_t *chain_par,
                               double w_stay, double w_step, double w_skip, double w_trim, int layers,
                               const int32_t *status_in, double *out_z, double *out_x, int32_t *out_status,
                               double *out_ms);

#ifdef __cplusplus
}
#endif
#endif /* NADAVCA_HIP_H */
