// Internal declarations shared by the HIP translation units of libnadavca_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "../../include/nadavca_hip.h"
#include "plan_key.h"

// ----- device-side tables ---------------------------------------------------------------
// One entry per DP row r of a read.  A "row" is a boundary line of the banded matrix
// (reference: one Node, nadavca/dtw/node.h:7-30); the density fields describe the STEP
// r -> r+1 (reference: distributions[r] / min_event_lengths[r], dtw.cpp:161-180).
// A constant density (transition rows, kmer_model.cpp:64-94) is stored as a Gaussian
// with mc = 0 and ac = the constant.
struct __attribute__((aligned(16))) RowParam {
  double mean, ac, mc;     // step r -> r+1 : e(x) = ac - (x-mean)^2 * mc
  int32_t bs, be;          // band of row r, inclusive sample-boundary indices
  int32_t lo, hi;          // lane occupancy of row r: band + warm-up/pre-roll on both sides
  int32_t mel;             // min event length of step r -> r+1
  int32_t off;             // per-row time offset: kernels_align3 computes cell (r, i) at step i + off[r]
};
static_assert(sizeof(RowParam) == 48, "RowParam layout");

// estimate_log_likelihoods: one entry per base position j of a sweep, describing the FUSED pair
// of reference rows handled by one lane: the wobble row (mixture density, min event length 0,
// dtw.cpp:53-59 / 70-76) on band "w", then the emitting row (Gaussian, dtw.cpp:60-63 / 77-80)
// on band "e".  Coordinates are those of the sweep (mirrored for the suffix sweep).
struct __attribute__((aligned(16))) FusedParam {
  double b_mean, b_ac, b_mc;  // the emitting Gaussian; the mixture's other component is the left neighbour's
  int32_t wbs, wbe;           // band of the wobble row == band of the predecessor row
  int32_t ebs, ebe;           // band of the emitting row
  int32_t has_wob;            // 0: no wobble row, the predecessor feeds the emitting row directly
  int32_t store_off;          // first cell of the emitting row in the slot's row store
};
static_assert(sizeof(FusedParam) == 48, "FusedParam layout");

struct ReadMeta {
  int64_t sig_off;   // first sample of the read's signal slice
  int64_t row_off;   // first RowParam of the read
  int64_t ref_off;   // first base (output offset)
  int32_t N;         // samples in the slice
  int32_t R;         // bases
  int32_t T;         // DP rows
  int32_t c;         // wavefront skew: cell (r,i) is computed at step t = i + c*r
  int32_t t_min;     // first step
  int32_t n_steps;   // number of steps
  int32_t status;    // NVK_READ_*
  int32_t pad;       // align planner: number of steps under the per-row offsets RowParam::off
  int64_t cells;     // sum of band widths (algorithmic cell count)
  int32_t cw;        // align planner: 0, or the skew of a read served by a TEAM of ALIGN3_TEAM_W waves
                     // (kernels_align3.hip: one row per lane of 64 * ALIGN3_TEAM_W lanes; RowParam::off = cw * r)
  int32_t rsv;       // align planner: 1 if two adjacent bases of the read have the same k-mer level (NVK_TIE_PLATEAU)
};

// totals reduced over a batch by the planner (read back once by the host)
struct PlanTotals {
  int32_t max_steps;
  int32_t n_wide;   // reads whose skew exceeds the main launch's cap
  int32_t max_c;
  int32_t max_T;
  int32_t max_W;
  int32_t max_cw;   // largest team skew (ReadMeta::cw)
  unsigned long long cells;
  unsigned long long steps;
};

struct DeviceModel {
  int k, central, alphabet;
  int64_t n;
  const double *mean, *ac, *mc;  // device arrays [n]
};

// ----- host-side objects ------------------------------------------------------------------
enum { WS_META = 0, WS_ROWS = 1, WS_BANDTMP = 2, WS_SPILL = 3, WS_BP = 4, WS_MISC = 5, WS_ROWS2 = 6, WS_STAGE = 7,
       WS_SPILL_B = 8, WS_STAGE_B = 9, WS_BP_B = 10, WS_LANE_F = 11, WS_LANE_R = 12, WS_ORDER = 13, WS_OFFS = 14, WS_TIES = 15, WS_RSTATE = 16, WS_STEPS = 17,
       WS_SEED_TB = 18, WS_SEED_OFF = 19, WS_JOINT = 20, WS_SEED_CHAIN = 21, WS_STATE_MOM = 22, WS_COUNT = 23 };

struct nvk_ctx {
  int device;
  hipStream_t stream;
  hipStream_t stream2;   // side stream: the wide-skew class of the exact align kernel runs here
  hipEvent_t ev_fork, ev_join;
  int slots_override;
  int num_cus;
  // growable workspaces (device)
  void *ws[WS_COUNT];
  size_t ws_bytes[WS_COUNT];
  // timing
  int timing_on;
  double k_ms[NVK_K_COUNT];
  int64_t k_launches[NVK_K_COUNT];
  hipEvent_t ev0, ev1;
  // stats of the last batch
  int64_t last_cells, last_steps, last_spill_bytes;
  // 1 while ws[WS_ROWS] holds the RowParam table of the batch planned last (plan_batch in api.hip clears it before it
  // plans and sets it when the planner wrote the table); the exact align kernel is launched only with it set
  int rows_current;
  int64_t last_retries;  // reads of the last refine batch redone by the exact kernel
  int64_t last_ties;     // reads of the last refine batch with a path decision inside the tie margin
  int64_t last_ties_exact, last_ties_near, last_ties_ulp;  // ... per class (NVK_TIE_EXACT / _NEAR / _ULP)
  // the tie flags of the last nvk_refine_alignment_batch[_dev] call (nvk_last_tie_flags): its number of reads, and
  // where they are: null = on the device in ws[WS_TIES], else the host copy of the pipelined path (pipeline.hip)
  int64_t ties_n;
  const int32_t *ties_host;
  // launch report (include/nadavca_hip.h): the launch classes of the last device-pointer refine / log-likelihood call
  // (nvk_launch_reset at its start, nvk_launch_note per class) and the number of reads whose ReadMeta that call left in
  // ws[WS_META] (nvk_last_read_skews; -1: none, or the table was taken by a later plan)
  nvk_launch_rec launches[NVK_LAUNCH_CAP];
  int n_launches;
  int64_t meta_n;
  int64_t ws_limit;      // nvk_ctx_set_workspace_limit: cap on the sweep kernels' spill workspace (0 = default)
  // one pinned host block the planner's results arrive in with ONE copy + synchronisation per batch: the totals,
  // then the reads' step counts in launch order (refine_alignment; sizes the spill slots)
  void *h_plan;
  size_t h_plan_cap;
  // The plan this ctx holds (plan_key.h): set when a keyed refine call has planned, while WS_META, WS_LANE_F,
  // WS_LANE_R, WS_OFFS, WS_ORDER, WS_STEPS, the device totals and h_plan still hold what its planner left; cleared by
  // whatever plans anew (plan_batch_queue, ell_run) or lets one of those blocks go (nvk_ws_reserve).  rows_current
  // goes on saying whether WS_ROWS holds that plan's row table.
  plan_key::Key plan_key;
  int plan_reused;       // the last refine call on this ctx swept from the held plan (nvk_last_plan_reused)
  int spill_share;       // > 1: this ctx is one of that many lanes of a pipelined host path sharing the device
  struct nvk_pipe_state *pipe;  // lanes of the pipelined host-pointer entry points (pipeline.hip), made on first use
};

// launch report: forget the last call's records (and its metas) / add one record, counted also beyond the capacity
inline void nvk_launch_reset(nvk_ctx *ctx) {
  ctx->n_launches = 0;
  ctx->meta_n = -1;
}
inline void nvk_launch_note(nvk_ctx *ctx, const nvk_launch_rec &r) {
  if (ctx->n_launches < NVK_LAUNCH_CAP) ctx->launches[ctx->n_launches] = r;
  ctx->n_launches++;
}

struct nvk_model {
  nvk_ctx *ctx;
  DeviceModel dm;
  double *d_mean, *d_ac, *d_mc;
  uint64_t id;  // process-wide, never reused: what a plan key names the model by
};


void nvk_set_error(const char *fmt, ...);
// pipeline.hip
void nvk_pipe_release(nvk_ctx *ctx);
void nvk_pipe_set_ws_limit(nvk_ctx *ctx, int64_t bytes);

// ----- allocation (api.hip) ------------------------------------------------------------------
// The one place device (pinned = false) and pinned host memory is allocated.  A failure leaves *p null, sets the
// error text (naming `what`), clears the thread's HIP last error — so that the launch checks after it see only
// their own errors — and returns NVK_ERR_NOMEM.
int nvk_alloc(void **p, size_t bytes, bool pinned, const char *what);
// grow-only buffer: nothing happens if bytes <= *cap; else the old block is freed and bytes + bytes/8 + 4096 are
// allocated, or exactly bytes if that fails
int nvk_grow(void **p, size_t *cap, size_t bytes, bool pinned, const char *what);
// ctx->ws[which] through nvk_grow, after both streams are drained (queued kernels may still use the old block)
int nvk_ws_reserve(nvk_ctx *ctx, int which, size_t bytes);

struct TimerScope {
  nvk_ctx *ctx;
  int id;
  bool stopped = false;
  TimerScope(nvk_ctx *c, int kid);
  // ends the timed interval here; the scope's end then only waits for it and reads it, so that host work between the
  // two runs beside the kernels with timing on as it does with timing off
  void stop();
  ~TimerScope();
};

#define NVK_HIP(call)                                                                  \
  do {                                                                                 \
    hipError_t _e = (call);                                                            \
    if (_e != hipSuccess) {                                                            \
      nvk_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__,   \
                    __LINE__);                                                         \
      return NVK_ERR_HIP;                                                              \
    }                                                                                  \
  } while (0)

// the close of an entry: `launch()` under a TimerScope of kernel class kid, then the launch error, then the stream
template <class Launch>
inline int nvk_timed(nvk_ctx *ctx, int kid, Launch &&launch) {
  {
    TimerScope ts(ctx, kid);
    launch();
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

// f(std::integral_constant<int, V>{}) for the V in LO .. HI that equals v: a run-time count as a template parameter;
// false, and no call, when v is outside
template <int LO, int HI, class F>
inline bool dispatch_int(int v, F &&f) {
  if constexpr (LO > HI) {
    return false;
  } else {
    if (v != LO) return dispatch_int<LO + 1, HI>(v, f);
    f(std::integral_constant<int, LO>{});
    return true;
  }
}

// scoped temporary device buffer of the host-pointer entry points: max(bytes, 16) bytes, filled from host src
// (when not null) on stream s, freed when it goes out of scope
struct NvkTmp {
  void *p = nullptr;
  ~NvkTmp() {
    if (p) (void)hipFree(p);
  }
  int up(const void *src, size_t bytes, hipStream_t s) {
    int rc = nvk_alloc(&p, bytes ? bytes : 16, false, "temporary");
    if (rc) return rc;
    if (bytes && src) NVK_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s));
    return NVK_OK;
  }
};

// the planner's totals on the device: in ws[WS_MISC] (at least 256 bytes once reserved), behind the launchers'
// 64 bytes of counters
inline PlanTotals *nvk_plan_totals(nvk_ctx *ctx) { return (PlanTotals *)((char *)ctx->ws[WS_MISC] + 64); }

// blocks for `items` work items at per_block each, clamped to a grid the grid-stride kernels cover any size with
inline unsigned grid_of(int64_t items, int64_t per_block) {
  const int64_t want = (items + per_block - 1) / per_block;
  return (unsigned)(want < 65535 * 16 ? want : 65535 * 16);
}

__device__ __forceinline__ double nvk_neg_inf() { return __longlong_as_double(0xfff0000000000000ll); }

// the read that owns flat position g: the rd with off[rd] <= g < off[rd + 1], by binary search over off[0..n]
__device__ __forceinline__ int64_t owner_of(const int64_t *off, int64_t n, int64_t g) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// lo + the first i in [0, n) with key[lo + i] >= want (lo + n if none); key ascending.  Stays in [lo, lo + n] for any
// key, sorted or not.
__device__ __forceinline__ int64_t lower_bound(const int64_t *key, int64_t lo, int64_t n, int64_t want) {
  int64_t hi = lo + n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ----- argument checks (api.hip) -------------------------------------------------------------
// off[0..n]: not NULL, starts at 0, never decreases
int check_offsets(const char *what, const int64_t *off, int64_t n);
// off[0..n] on the DEVICE: copied to h_off over ctx->stream (which is waited for) and checked there with
// check_offsets; with total_name, the offsets must also end at `total`, the argument of that name
int nvk_fetch_offsets(nvk_ctx *ctx, const char *what, const int64_t *off, int64_t n, std::vector<int64_t> &h_off,
                      const char *total_name = nullptr, int64_t total = 0);
// log costs: every value of v finite and <= 0, else an error "<what>: <names> is not ..." with `names` a printf
// format that takes the values as %g, in order (at most four)
int check_log_costs(const char *what, const char *names, std::initializer_list<double> v);
// the model handle and the ranges of n_reads, bandwidth and min_event_length
int check_common(nvk_model *model, int64_t n_reads, int bandwidth, int mel);
// the per-site two-sample entries (nvk_site_rank_tests_dev, nvk_site_mixture_tests_dev): ctx, the three counts >= 0
// and, with n_sites > 0 only, site_key and the key and values of a sample that has rows (an empty sample may be NULL)
int check_site_samples(const char *what, nvk_ctx *ctx, int64_t n_rows_a, const int64_t *key_a, const double *val_a,
                       int64_t n_rows_b, const int64_t *key_b, const double *val_b, int64_t n_sites,
                       const int64_t *site_key);
// the per-read row entries (read_rows.h): ctx, n_reads in 0 .. 2^31-1, total_ref >= 0 and 0 with no reads; ref_off on
// the device, fetched, checked and ending at total_ref; every array of `arrays` with its offsets fetched and checked,
// its data NULL only when they end at 0.  *nothing_to_do: the checks passed and there is no base to serve.
struct ReadRowsArray { const char *name; const int64_t *off; const void *data; };
int check_read_rows(const char *what, nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int64_t *ref_off,
                    std::initializer_list<ReadRowsArray> arrays, bool *nothing_to_do);

// ----- launchers (kernels_*.hip) ------------------------------------------------------------
struct BatchArgs {
  int64_t n_reads, total_signal, total_ref, total_anchors;
  const double *signal;
  const int64_t *sig_off;
  const int32_t *reference;
  const int64_t *ref_off;
  const int32_t *ctx_before;
  const int64_t *cb_off;
  const int32_t *ctx_after;
  const int64_t *ca_off;
  const int32_t *anchors;
  const int64_t *anc_off;
  int bandwidth, mel;
};

enum { PLAN_ALIGN_TRANS = 0, PLAN_ALIGN_PLAIN = 1 };

// lane_f / lane_r / lane_offs: where the planner leaves the per-sweep lane records of kernels_align3.hip (lane3.h),
// or null.  write_rows: whether the RowParam table is written — only the exact kernel (launch_align,
// launch_align_retry) reads it; without it `rows` is left unwritten, for every read.  totals == null: a second pass over a batch already planned, which leaves
// the device totals alone and rewrites the metas with the values they have.  meanwhile (or null): host work of the
// caller that depends on nothing the planner finds, called once the planner is queued, so that it runs beside it.
int launch_plan(nvk_ctx *ctx, const DeviceModel &dm, const BatchArgs &a, int mode,
                ReadMeta *metas, RowParam *rows, unsigned long long *bandtmp, PlanTotals *totals,
                void *lane_f, void *lane_r, int32_t *lane_offs, int write_rows,
                const std::function<int()> *meanwhile = nullptr);
// order[0..n) = read indices in launch order (class-major, longest first; ctx->ws[WS_ORDER]); tot_dev: the planner's
// totals on the device; steps_out (device, n ints, or null): the reads' step counts in that order
int launch_order(nvk_ctx *ctx, const ReadMeta *metas, int64_t n_reads, const PlanTotals *tot_dev, int **order,
                 int32_t *steps_out);
int launch_align(nvk_ctx *ctx, const BatchArgs &a, int transitions, const ReadMeta *metas,
                 const RowParam *rows, const PlanTotals &tot, int32_t *out_events,
                 int32_t *out_status);
struct EllPlan {
  ReadMeta *metas;
  FusedParam *fwd;       // [total_ref] prefix-sweep descriptors, position order
  FusedParam *rev;       // [total_ref] suffix-sweep descriptors, mirrored coordinates
  int32_t *bs, *be;      // [total_ref + n] bands per boundary row
  int32_t *rowoff;       // [total_ref + n] offset of each boundary row in the row store
};
int launch_plan_ell(nvk_ctx *ctx, const DeviceModel &dm, const BatchArgs &a, int wobbling,
                    const EllPlan &pl, unsigned long long *bandtmp, PlanTotals *totals);
// What a launch of ell_kernel scores.  Full: every substitution of every position, into out_ll; nothing below `kind`
// is read.  The other kinds: read j's hypotheses off[j] .. off[j+1] of a list, into out_total / out_hyp (out_ll
// unused), the list being the kind's own struct — which is also what its kernels take as their argument.
enum class EllKind { Full = NVK_ELL_FULL, Listed = NVK_ELL_LISTED, Joint = NVK_ELL_JOINT, Edit = NVK_ELL_EDIT };
// Listed (nvk_estimate_hypotheses_batch_dev): hypothesis h is the substitution (pos[h], base[h])
struct EllListed { const int32_t *pos, *base; };
// Joint (.._joint_hypotheses_..): hypothesis h is the substitutions sub_off[h] .. sub_off[h+1] of (sub_pos, sub_base)
struct EllJoint { const int64_t *sub_off; const int32_t *sub_pos, *sub_base; };
// Edit (.._edit_hypotheses_..): h deletes del[h] bases from pos[h] on and inserts ins_off[h] .. ins_off[h+1] of ins_base
struct EllEdit { const int32_t *pos, *del; const int64_t *ins_off; const int32_t *ins_base; };
struct EllList {  // what the three listed kinds share
  const int64_t *off = nullptr;
  double *out_total = nullptr;  // [n_reads]
  double *out_hyp = nullptr;    // [off[n_reads]]
  int64_t total_hyp = 0;        // off[n_reads]; Joint and Edit keep one item per hypothesis in WS_JOINT
};
struct EllHyp {
  EllKind kind = EllKind::Full;
  EllList list;
  EllListed listed = {};  // the list of `kind`:
  EllJoint joint = {}; EllEdit edit = {};
};
int launch_ell(nvk_ctx *ctx, const DeviceModel &dm, const BatchArgs &a, int wobbling,
               const EllPlan &pl, const PlanTotals &tot, double *out_ll, int32_t *out_status, const EllHyp &hyp);
// out_count[0..4) = number of entries of flags[0..n) that are nonzero / have bit 0 / bit 1 / bit 2 set
int launch_count_flags(nvk_ctx *ctx, const int32_t *flags, int64_t n, int32_t *out_count);
// bytes the resident waves' spill may take: the ctx limit if set, else a default share of the free memory
int64_t nvk_spill_cap(nvk_ctx *ctx, int which_ws);
// internal per-read status of the scaled-double kernel: the exact kernel must redo this read
constexpr int NVK_READ_RETRY_INTERNAL = 2;
constexpr int ALIGN3_TEAM_W = 4;  // waves per read for wide bands (skew above ALIGN1_C_CAP with one wave)
constexpr int ALIGN1_C_CAP = 3;  // skew served by the main launch of the one-read-per-wave kernel
// only_retry != 0: serve only the reads whose out_status is NVK_READ_RETRY_INTERNAL
int launch_align_retry(nvk_ctx *ctx, const BatchArgs &a, int transitions, const ReadMeta *metas,
                       const RowParam *rows, const PlanTotals &tot, int32_t *out_events,
                       int32_t *out_status);
// scaled-double kernel (kernels_align3.hip).  order / steps_sorted: launch order (device) and the reads' step counts
// in that order (host), from plan_batch_queue / plan_batch_wait (api.hip); d_retry (device int, zero in stream order before this call): reads it
// hands to the exact kernel.  Asynchronous: nothing is waited for.
// What the sweeps need that depends neither on the planner's totals nor on the step counts is set up by the two calls
// before it, so that the host does it while the planner runs and not between the planner's end and the first sweep:
//   align3_reserve   the workspaces sized by the batch alone; before the planner is queued (a workspace that grows
//                    drains the stream first)
//   align3_prepare   queues the zeroing of the sweep counters and asks for the spill cap (*spill_cap: the bytes the
//                    first class's chunks may take); after every workspace of the planner is reserved
int align3_reserve(nvk_ctx *ctx, int64_t n_reads);
int align3_prepare(nvk_ctx *ctx, int64_t *spill_cap);
int launch_align3(nvk_ctx *ctx, const BatchArgs &a, int transitions, const ReadMeta *metas, const PlanTotals &tot,
                  const int *order, const int32_t *steps_sorted, int32_t *out_events, int32_t *out_status,
                  int *d_retry, int64_t spill_cap);
int launch_expected(nvk_ctx *ctx, const DeviceModel &dm, int64_t n_reads, int64_t total_ref,
                    const int32_t *reference, const int64_t *ref_off, const int32_t *cb,
                    const int64_t *cb_off, const int32_t *ca, const int64_t *ca_off, double *out);
