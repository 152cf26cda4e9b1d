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

namespace {

constexpr int NT = 256;
constexpr int MAX_K = 16;  // longest k-mer whose key fits the checks below (alphabet^k <= 2^31)

// ---- numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, @TYPE@_pairwise_sum) ------
// The same order as np_sum in kernels_renorm.hip, over a generated sequence f(0 .. n) instead of an array (the
// squared deviations of pass 2 and the values of the reduction are never stored), and with the walk's stack in
// registers: every access to it is an unrolled select over its 8 frames, so it needs no scratch memory.
// Resource use (gfx950, -Rpass-analysis=kernel-resource-usage): kmer_event_kernel 72 / 74 VGPRs and 72 / 74 SGPRs
// (pass 1 / pass 2), long_event_kernel 82 / 84 VGPRs and 99 / 101 SGPRs, kmer_reduce_kernel 86 VGPRs and 99 SGPRs;
// no LDS, no scratch, no spills.
template <class F>
__device__ __forceinline__ double np_block_sum(const F &f, int o, int n) {  // n <= 128
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; i++) res += f(o + i);
    return res;
  }
  double r0 = f(o + 0), r1 = f(o + 1), r2 = f(o + 2), r3 = f(o + 3);
  double r4 = f(o + 4), r5 = f(o + 5), r6 = f(o + 6), r7 = f(o + 7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += f(o + i + 0); r1 += f(o + i + 1); r2 += f(o + i + 2); r3 += f(o + i + 3);
    r4 += f(o + i + 4); r5 += f(o + i + 5); r6 += f(o + i + 6); r7 += f(o + i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; i++) res += f(o + i);
  return res;
}

__device__ __forceinline__ int np_split(int m) {  // left half of a node of m > 128 elements
  int n2 = m / 2;
  return n2 - n2 % 8;
}

// sum(a, n) = sum(a, n2) + sum(a + n2, n - n2) down to blocks of <= 128, n <= 8192: a node of m elements has
// children of at most m/2 + 8, so a path from the root holds at most 7 internal nodes.  The walk keeps the path as
// bits (bit i: the node at depth i + 1 is a right child), rebuilds a node's offset and size from them when it needs
// them, and keeps the left sums of the path's nodes in sv.
template <class F>
__device__ double np_pairwise_sum(const F &f, int o0, int n) {
  if (n <= 128) return np_block_sum(f, o0, n);
  constexpr int D = 8;
  double sv[D];
#pragma unroll
  for (int i = 0; i < D; i++) sv[i] = 0.0;
  unsigned path = 0;
  int d = 0, o = o0, m = n;  // the current node and its depth
  for (;;) {
    while (m > 128) {  // descend left
      m = np_split(m);
      path &= ~(1u << d);
      d++;
    }
    double ret = np_block_sum(f, o, m);
    for (;;) {  // ascend until a node still has its right child to do
      if (d == 0) return ret;
      d--;
      if (!((path >> d) & 1u)) {  // the left child of the node at depth d is done: keep it, go right
#pragma unroll
        for (int i = 0; i < D; i++)
          if (i == d) sv[i] = ret;
        int po = o0, pm = n;
        for (int i = 0; i < d; i++) {
          const int n2 = np_split(pm);
          if ((path >> i) & 1u) { po += n2; pm -= n2; } else { pm = n2; }
        }
        const int n2 = np_split(pm);
        path |= 1u << d;
        d++;
        o = po + n2;
        m = pm - n2;
        break;
      }
      double pv = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++)
        if (i == d) pv = sv[i];
      ret = pv + ret;
    }
  }
}

// numpy.add.reduce of a contiguous float64 vector: pieces of 8192 (numpy's buffer), each summed pairwise and added to
// the running result, which starts at 0 (as np_sum in kernels_renorm.hip; tests/test_renorm_cpu.py)
template <class F>
__device__ double np_sum(const F &f, int64_t n) {
  double res = 0.0;
  for (int64_t o = 0; o < n; o += 8192) {
    const int64_t base = o;
    auto g = [&](int i) { return f(base + i); };
    res = res + np_pairwise_sum(g, 0, (int)(n - o < 8192 ? n - o : 8192));
  }
  return res;
}

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
    const int32_t *ref = reference + r0, *cb = ctx_before + cb_off[rd] + B, *ca = ctx_after + ca_off[rd] - R;
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
        if (e > s) {
          key = 0;
          for (int m = 0; m < k; m++) {
            const int p = p0 + m;
            const int32_t b = p < 0 ? cb[p] : (p < R ? ref[p] : ca[p]);
            if (b < 0 || b >= alphabet) {
              key = -1;
              break;
            }
            key = key * alphabet + b;
          }
        }
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
    int64_t lo = 0, hi = n_reads;  // ref_off[lo] <= g < ref_off[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (ref_off[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t N = sig_off[lo + 1] - sig_off[lo];
    int64_t s = events[2 * g];
    s = s < 0 ? 0 : (s > N ? N : s);
    out_val[g] = event_value<PASS2>(signal + sig_off[lo] + s, len[g], level, key[g]);
  }
}

// lo + the first i in [0, n) with key[lo + i] >= want (lo + n if none); key ascending.  Stays in [lo, lo + n] for any
// key, sorted or not.
__device__ int64_t lower_bound(const int64_t *key, int64_t lo, int64_t n, int64_t want) {
  int64_t hi = lo + n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
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

unsigned grid_of(int64_t items, int64_t per_block) {
  const int64_t want = (items + per_block - 1) / per_block;
  return (unsigned)(want < 65535 * 16 ? want : 65535 * 16);
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

int copy_check(nvk_ctx *ctx, const char *what, const int64_t *d_off, int64_t n_reads, std::vector<int64_t> &off) {
  off.resize((size_t)n_reads + 1);
  NVK_HIP(hipMemcpyAsync(off.data(), d_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return check_offsets(what, off.data(), n_reads);
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
  if ((rc = copy_check(ctx, "reference", ref_off, n_reads, off))) return rc;
  if (off[n_reads] != total_ref) {
    nvk_set_error("%s: reference offsets end at %lld, total_ref is %lld", what, (long long)off[n_reads],
                  (long long)total_ref);
    return NVK_ERR_INVALID;
  }
  if ((rc = copy_check(ctx, "signal", sig_off, n_reads, off))) return rc;
  if (off[n_reads] > 0 && !signal) {
    nvk_set_error("%s: signal is NULL", what);
    return NVK_ERR_INVALID;
  }
  if ((rc = copy_check(ctx, "context_before", cb_off, n_reads, off))) return rc;
  if (off[n_reads] > 0 && !ctx_before) {
    nvk_set_error("%s: context_before is NULL", what);
    return NVK_ERR_INVALID;
  }
  if ((rc = copy_check(ctx, "context_after", ca_off, n_reads, off))) return rc;
  if (off[n_reads] > 0 && !ctx_after) {
    nvk_set_error("%s: context_after is NULL", what);
    return NVK_ERR_INVALID;
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
