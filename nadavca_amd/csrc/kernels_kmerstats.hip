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
// Work split of the event pass: ONE WAVE PER READ, its lanes over the read's events 64 at a time.  A read's
// offsets and status are wave-uniform (scalar loads, no per-thread binary search for the owner as in
// event_means_kernel), and a read that did not align is skipped by the whole wave without touching its samples.
// Lane l of a step takes event l, so at every step of the sample loop the wave's 64 loads fall in one contiguous run
// of about 64 events' samples (10 samples, 80 B, per event in practice): each cache line it fetches serves the
// neighbouring lanes in the same and the following steps.  Events are 3 to 17 samples long, so lanes of a step
// finish at different times; that divergence is inherent to exact per-event sums and costs VALU issue slots, not
// bytes, in a pass whose time is the signal's 8 B per sample.  Idle lanes in a read's last step of 64 cost about
// 1/12 of a 400-base read.  An event of more than 128 samples takes numpy's pairwise walk; it is rare, and
// long_event_kernel sums it after the main pass, so the main kernel's registers hold no walk state (it ran out of
// scalar registers with it).
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

namespace {

constexpr int NT = 256;
constexpr int MAX_K = 16;  // longest k-mer whose key fits the checks below (alphabet^k <= 2^31)

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

// one wave per read (grid-stride), its lanes over the read's events; PASS2: level != null.  An event of more than 128
// samples (numpy's pairwise walk; rare: events are 3 to 17 samples in practice) gets its key and length here and its
// value from long_event_kernel, so that this kernel's registers hold no walk state.
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
    if (status && status[rd] != 0) {
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
    const int32_t *ev = events + 2 * r0;
    for (int g = lane; g < R; g += 64) {
      int64_t key = -1;
      int len = 0;
      double val = 0.0;
      const int p0 = g - central;  // first base of the window, reference-part coordinates
      if (g >= trim && g < R - trim && p0 >= -B && p0 + k - 1 < R + A) {
        int s = ev[2 * g], e = ev[2 * g + 1];
        s = s < 0 ? 0 : (s > N ? N : s);  // numpy slice clamping, as event_means_kernel
        e = e < 0 ? 0 : (e > N ? N : e);
        if (e > s) key = kmer_id_checked(dm, ref, R, cb, B, ca, A, g);
        if (key >= 0) {
          len = e - s;
          if (len <= 128) val = event_value<PASS2>(x + s, len, level, key);  // else: long_event_kernel
        }
      }
      out_key[r0 + g] = key;
      out_val[r0 + g] = val;
      out_len[r0 + g] = len;
    }
  }
}

// the values of the counted events of more than 128 samples: one thread per event, the read found by a binary search
template <bool PASS2>
__global__ __launch_bounds__(NT) void long_event_kernel(int64_t n_reads, int64_t total_ref, const double *signal,
                                                        const int64_t *sig_off, const int32_t *events,
                                                        const int64_t *ref_off, const double *level,
                                                        const int64_t *key, const int64_t *len, double *out_val) {
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < total_ref; g += (int64_t)gridDim.x * NT) {
    if (key[g] < 0 || len[g] <= 128) continue;
    const int64_t lo = owner_of(ref_off, n_reads, g);
    const int64_t N = sig_off[lo + 1] - sig_off[lo];
    int64_t s = events[2 * g];
    s = s < 0 ? 0 : (s > N ? N : s);
    out_val[g] = event_value<PASS2>(signal + sig_off[lo] + s, len[g], level, key[g]);
  }
}

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

// alphabet^k, or -1 when k / alphabet are outside the served range
int64_t table_size(int k, int alphabet) {
  if (k < 1 || k > MAX_K || alphabet < 1 || alphabet > 64) return -1;
  int64_t n = 1;
  for (int i = 0; i < k; i++) {
    n *= alphabet;
    if (n > ((int64_t)1 << 31)) return -1;
  }
  return n;
}

}  // namespace

extern "C" int nvk_kmer_event_stats_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                                        const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                                        const int32_t *reference, const int32_t *ctx_before, const int64_t *cb_off,
                                        const int32_t *ctx_after, const int64_t *ca_off, const int32_t *status,
                                        int k, int central, int alphabet, int trim, const double *level,
                                        int64_t *out_key, double *out_val, int64_t *out_len) {
  const char *what = "nvk_kmer_event_stats_dev";
  if (!ctx || n_reads < 0 || n_reads > 0x7fffffff || total_ref < 0) {
    nvk_set_error("%s: invalid argument", what);
    return NVK_ERR_INVALID;
  }
  if (table_size(k, alphabet) < 0 || central < 0 || central >= k || trim < 0) {
    nvk_set_error("%s: k %d, central %d, alphabet %d, trim %d outside the served range (1 <= k, 0 <= central < k, "
                  "alphabet^k <= 2^31, trim >= 0)", what, k, central, alphabet, trim);
    return NVK_ERR_INVALID;
  }
  if (n_reads == 0) {
    if (total_ref != 0) {
      nvk_set_error("%s: total_ref %lld with no reads", what, (long long)total_ref);
      return NVK_ERR_INVALID;
    }
    return NVK_OK;
  }
  if (!sig_off || !ref_off || !cb_off || !ca_off) {
    nvk_set_error("%s: offsets are NULL", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  int rc;
  if ((rc = nvk_fetch_offsets(ctx, "reference", ref_off, n_reads, off, "total_ref", total_ref))) return rc;
  // (a data array may be NULL only when its offsets end at 0)
  const struct { const char *name; const int64_t *off; const void *data; } arr[3] = {
      {"signal", sig_off, signal}, {"context_before", cb_off, ctx_before}, {"context_after", ca_off, ctx_after}};
  for (const auto &x : arr) {
    if ((rc = nvk_fetch_offsets(ctx, x.name, x.off, n_reads, off))) return rc;
    if (off[n_reads] > 0 && !x.data) {
      nvk_set_error("%s: %s is NULL", what, x.name);
      return NVK_ERR_INVALID;
    }
  }
  if (total_ref == 0) return NVK_OK;
  if (!events || !reference || !out_key || !out_val || !out_len) {
    nvk_set_error("%s: NULL events, reference or output", what);
    return NVK_ERR_INVALID;
  }
  {
    TimerScope ts(ctx, NVK_K_KMER);
    auto event_kernel = level ? kmer_event_kernel<true> : kmer_event_kernel<false>;
    auto long_kernel = level ? long_event_kernel<true> : long_event_kernel<false>;
    hipLaunchKernelGGL(event_kernel, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads, signal,
                       sig_off, events, ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k, central,
                       alphabet, trim, level, out_key, out_val, out_len);
    hipLaunchKernelGGL(long_kernel, dim3(grid_of(total_ref, NT)), dim3(NT), 0, ctx->stream, n_reads, total_ref, signal,
                       sig_off, events, ref_off, level, (const int64_t *)out_key, (const int64_t *)out_len, out_val);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
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
  {
    TimerScope ts(ctx, NVK_K_KMER);
    hipLaunchKernelGGL(kmer_reduce_kernel, dim3(grid_of(n_kmers, NT)), dim3(NT), 0, ctx->stream, n_events, n_kmers,
                       key, val, len, out_sum, out_samples, out_events);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
