// The M-step of k-mer table training (nadavca_amd/kmer_train.py): per-k-mer sample statistics over the final events
// of an aligned batch, exact and deterministic (the contract: include/nadavca_hip.h, nvk_kmer_event_stats_dev).
//
//   nvk_kmer_event_stats_dev   per event: its k-mer key, its sample count and np.sum of its samples (pass 1) or of
//                              their squared deviations from the k-mer's level (pass 2)
//   nvk_kmer_reduce_dev        per k-mer: np.sum of its events' values in stable key order (the caller sorts and
//                              gathers), and the integer sample and event counts
//
// No floating-point atomics anywhere: every sum is one thread's loop in numpy's pairwise order, so the results equal
// numpy's bit for bit and are the same on every run.  The caller sorts the keys (a stable sort is plumbing).
//
// Work split of the event pass: one wave per read, its lanes over the read's events, and a second pass for the rare
// event of more than 128 samples (read_rows.h explains both).  The pass's time is the signal's 8 B per sample.
//
// Work split of the reduction: ONE THREAD PER K-MER, over its events' values laid out contiguously in sorted order (the
// caller gathers them after the sort: plumbing), so a thread's 8 interleaved chains of numpy's order read one cache
// line per step.  A k-mer's cost grows with its event count, and the pass takes as long as the most frequent k-mer
// needs; a 4^6 table has only 4 096 threads.  If the statistics ever weigh against the alignment, split each k-mer's
// pairwise tree over a wave (its leaves of <= 128 events are independent).
#include <math.h>

#include <vector>

#include "nvk_internal.h"
#include "kmer.h"
#include "npsum.h"
#include "read_rows.h"

namespace {

constexpr int NT = 256;

// the value of one counted event of n samples at xs: np.sum of the samples (pass 1) or of their squared deviations
// from the k-mer's level (pass 2)
template <bool PASS2>
__device__ __forceinline__ double event_value(const double *xs, int64_t n, const double *level, int64_t key) {
  if (PASS2) {
    const double mu = level[key];
    auto f = [&](int64_t i) { const double dv = xs[i] - mu; return dv * dv; };
    return n <= 128 ? np_block_sum(f, 0, (int)n) : np_sum(f, n);
  }
  auto f = [&](int64_t i) { return xs[i]; };
  return n <= 128 ? np_block_sum(f, 0, (int)n) : np_sum(f, n);
}

// one wave per read (grid-stride), its lanes over the read's events: the pass of read_rows.h with the loop written out
// here (through for_each_read it took 12 fewer registers, and pass 2 over 10 000 reads ran 2 % slower in each of ten
// alternating runs: DESIGN.md 5.4).  PASS2: level != null.  An event of more than 128 samples gets its key and length
// here and its value from the second pass.  A read that did not align gets -1 / 0 / 0 for its bases, and its samples
// and contexts are not looked at.
template <bool PASS2>
__global__ __launch_bounds__(NT) void kmer_event_kernel(int64_t n_reads, const double *signal, const int64_t *sig_off,
                                                        const int32_t *events, const int64_t *ref_off,
                                                        const int32_t *reference, const int32_t *ctx_before,
                                                        const int64_t *cb_off, const int32_t *ctx_after,
                                                        const int64_t *ca_off, const int32_t *status, int k,
                                                        int central, int alphabet, int trim, const double *level,
                                                        int64_t *out_key, double *out_val, int64_t *out_len) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  const DeviceModel dm{k, central, alphabet, 0, nullptr, nullptr, nullptr};  // (kmer.h reads the window's shape only)
  for (int64_t rd = (int64_t)blockIdx.x * (NT / 64) + threadIdx.x / 64; rd < n_reads; rd += waves) {
    if (status && status[rd] != NVK_READ_OK) {
      for (int64_t g = ref_off[rd] + lane; g < ref_off[rd + 1]; g += 64) {
        out_key[g] = -1;
        out_val[g] = 0.0;
        out_len[g] = 0;
      }
      continue;
    }
    // the read's arrays; sizes of one read fit 32 bits (the C-ABI's reads are below 2^31 samples and bases)
    const int64_t r0 = ref_off[rd];
    const int R = (int)(ref_off[rd + 1] - r0);
    const double *x = signal + sig_off[rd];
    const int N = (int)(sig_off[rd + 1] - sig_off[rd]);
    const int B = (int)(cb_off[rd + 1] - cb_off[rd]);
    const int A = (int)(ca_off[rd + 1] - ca_off[rd]);
    const int32_t *ref = reference + r0, *cb = ctx_before + cb_off[rd], *ca = ctx_after + ca_off[rd];
    for (int g = lane; g < R; g += 64) {
      int64_t key = -1;
      int len = 0;
      double val = 0.0;
      if (counted_base(g, R, trim) && window_inside(g, k, central, R, B, A)) {
        int s, e;
        event_span(events + 2 * r0, g, N, s, e);
        if (e > s) key = kmer_id_checked(dm, ref, R, cb, B, ca, A, g);
        if (key >= 0) {
          len = e - s;
          if (len <= 128) val = event_value<PASS2>(x + s, len, level, key);  // else: the second pass
        }
      }
      out_key[r0 + g] = key;
      out_val[r0 + g] = val;
      out_len[r0 + g] = len;
    }
  }
}

// the second pass (long_event_kernel): the value of a counted event of more than 128 samples
template <bool PASS2>
struct LongEventValue {
  const double *level;
  const int64_t *key, *len;
  double *out_val;
  __device__ int64_t length(int64_t g) const { return len[g]; }
  __device__ void operator()(int64_t g, const double *xs, int64_t n) const {
    out_val[g] = event_value<PASS2>(xs, n, level, key[g]);
  }
};

// one thread per k-mer: np.sum of its events' values (contiguous, in sorted order), the sample and event counts
__global__ __launch_bounds__(NT) void kmer_reduce_kernel(int64_t n_events, int64_t n_kmers, const int64_t *key,
                                                         const double *val, const int64_t *len, double *out_sum,
                                                         int64_t *out_samples, int64_t *out_events) {
  for (int64_t km = (int64_t)blockIdx.x * NT + threadIdx.x; km < n_kmers; km += (int64_t)gridDim.x * NT) {
    const int64_t lo = lower_bound(key, 0, n_events, km);
    const int64_t hi = lower_bound(key, lo, n_events - lo, km + 1);
    const double *v = val + lo;
    const double s = np_sum([&](int64_t i) { return v[i]; }, hi - lo);
    int64_t ns = 0;
    for (int64_t i = lo; i < hi; i++) ns += len[i];
    out_sum[km] = s;
    out_samples[km] = ns;
    out_events[km] = hi - lo;
  }
}

}  // namespace

extern "C" int nvk_kmer_event_stats_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                                        const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                                        const int32_t *reference, const int32_t *ctx_before, const int64_t *cb_off,
                                        const int32_t *ctx_after, const int64_t *ca_off, const int32_t *status,
                                        int k, int central, int alphabet, int trim, const double *level,
                                        int64_t *out_key, double *out_val, int64_t *out_len) {
  const char *what = "nvk_kmer_event_stats_dev";
  if (kmer_table_size(k, alphabet) < 0 || central < 0 || central >= k || trim < 0) {
    nvk_set_error("%s: k %d, central %d, alphabet %d, trim %d outside the served range (1 <= k, 0 <= central < k, "
                  "alphabet^k <= 2^31, trim >= 0)", what, k, central, alphabet, trim);
    return NVK_ERR_INVALID;
  }
  bool nothing;
  int rc = check_read_rows(what, ctx, n_reads, total_ref, ref_off, {{"signal", sig_off, signal},
                           {"context_before", cb_off, ctx_before}, {"context_after", ca_off, ctx_after}}, &nothing);
  if (rc || nothing) return rc;
  if (!events || !reference || !out_key || !out_val || !out_len) {
    nvk_set_error("%s: NULL events, reference or output", what);
    return NVK_ERR_INVALID;
  }
  return nvk_timed(ctx, NVK_K_KMER, [&] {
    const dim3 rows(grid_of(n_reads, NT / 64)), longs(grid_of(total_ref, NT)), block(NT);
    dispatch_int<0, 1>(level != nullptr, [&](auto pass2) {
      constexpr bool PASS2 = decltype(pass2)::value;
      hipLaunchKernelGGL(kmer_event_kernel<PASS2>, rows, block, 0, ctx->stream, n_reads, signal, sig_off, events,
                         ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k, central, alphabet, trim,
                         level, out_key, out_val, out_len);
      hipLaunchKernelGGL(long_event_kernel, longs, block, 0, ctx->stream, n_reads, total_ref, signal, sig_off, events,
                         ref_off, (const int64_t *)out_key,
                         LongEventValue<PASS2>{level, out_key, out_len, out_val});
    });
  });
}

extern "C" int nvk_kmer_reduce_dev(nvk_ctx *ctx, int64_t n_events, int64_t n_kmers, const int64_t *key,
                                   const double *val, const int64_t *len, double *out_sum, int64_t *out_samples,
                                   int64_t *out_events) {
  const char *what = "nvk_kmer_reduce_dev";
  if (!ctx || n_events < 0 || n_kmers < 0 || n_kmers > ((int64_t)1 << 31)) {
    nvk_set_error("%s: invalid argument (0 <= n_kmers <= 2^31, n_events >= 0)", what);
    return NVK_ERR_INVALID;
  }
  if (n_kmers == 0) return NVK_OK;
  if (!out_sum || !out_samples || !out_events || (n_events > 0 && (!key || !val || !len))) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  return nvk_timed(ctx, NVK_K_KMER, [&] {
    hipLaunchKernelGGL(kmer_reduce_kernel, dim3(grid_of(n_kmers, NT)), dim3(NT), 0, ctx->stream, n_events, n_kmers,
                       key, val, len, out_sum, out_samples, out_events);
  });
}
