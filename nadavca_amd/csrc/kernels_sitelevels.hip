// Model-free per-site summaries (nadavca_amd/site_levels.py): the pile-up of the reads' event levels over every
// reference position and strand, as moments that can be saved, merged and tested between two samples (the contract:
// include/nadavca_hip.h, nvk_site_level_rows_dev).
//
//   nvk_site_level_rows_dev   per (read, base): its (global position, strand) as a sort key and four values of its
//                             event: level = np.mean, stdv = np.std, dwell, resid = level - expected level
//   nvk_site_moments_dev      per key: its number of rows and, per column, their mean and their sum of squared
//                             deviations from it, over the key's rows in stable key order (the caller sorts and
//                             gathers: plumbing)
//
// No floating-point atomics: an event's sums are one thread's loop in numpy's pairwise order (npsum.h), a key's sums
// are a lane's loop over its rows in ascending order followed by a butterfly over the wave.  Two runs give the same
// bits, and the numpy restatement of the tests gives them too.
//
// Work split of the row pass: ONE WAVE PER READ, its lanes over the read's bases 64 at a time, as kmer_event_kernel:
// offsets, status, strand and start are wave-uniform, and at every step of the sample loop the wave's loads fall in one
// run of about 64 events' samples.  A lane reads its event twice, once for the sum and once for the squared
// deviations; the second pass hits the lines the first one fetched, so the pass moves the signal's 8 B per sample from
// memory once, plus 8 B of events and 8 B of expected level in and 40 B out per base.  An event of more than 128
// samples takes numpy's pairwise walk; site_long_event_kernel serves it after the main pass, as long_event_kernel
// does for the k-mer statistics, so that the main kernel's registers hold no walk state.
//
// Work split of the moments: ONE WAVE PER KEY (grid-stride).  The key's rows are contiguous after the sort; their
// range comes from two wave-uniform binary searches, lane l takes rows l, l + 64, ..., and the n_val columns are
// reduced side by side (wave_sum_n: one shuffle's latency hides behind the others').  Two sweeps over the rows: the
// sums, then the squared deviations from the mean; the second sweep's rows are in cache.  A key of c rows keeps
// min(c, 64) lanes busy; at sequencing coverage most of the wave idles, which is the price of sums whose order does
// not depend on the launch.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.5.
#include <math.h>

#include <vector>

#include "nvk_internal.h"
#include "npsum.h"
#include "wave.h"

namespace {

constexpr int NT = 256;
constexpr int NCOL = 4;  // level, stdv, dwell, resid

// np.mean and np.std of the n samples at xs: numpy's pairwise sum and one division; then the rounded deviations, their
// rounded squares, numpy's pairwise sum of those, one division and the square root
template <bool LONG>
__device__ __forceinline__ void event_level_stdv(const double *xs, int64_t n, double &level, double &stdv) {
  auto f = [&](int64_t i) { return xs[i]; };
  const double s = LONG ? np_sum(f, n) : np_block_sum(f, 0, (int)n);
  const double m = s / (double)n;
  auto q = [&](int64_t i) { const double d = xs[i] - m; return d * d; };
  const double ss = LONG ? np_sum(q, n) : np_block_sum(q, 0, (int)n);
  level = m;
  stdv = sqrt(ss / (double)n);
}

// one wave per read (grid-stride), its lanes over the read's bases.  An event of more than 128 samples gets its key
// and dwell here and level, stdv and resid from site_long_event_kernel.
__global__ __launch_bounds__(NT) void site_rows_kernel(int64_t n_reads, const double *signal, const int64_t *sig_off,
                                                       const int32_t *events, const int64_t *ref_off,
                                                       const double *expected, const int64_t *chunk_start,
                                                       const int32_t *reverse, const int32_t *status, int trim,
                                                       int64_t ref_len, int64_t *out_key, double *out_val) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t rd = (int64_t)blockIdx.x * (NT / 64) + wave; rd < n_reads; rd += waves) {
    const int64_t r0 = ref_off[rd];
    const int64_t R = ref_off[rd + 1] - r0;
    if (R <= 0) continue;
    const bool live = !status || status[rd] == NVK_READ_OK;
    const double *x = signal + sig_off[rd];
    const int64_t N = sig_off[rd + 1] - sig_off[rd];
    const bool rev = reverse[rd] != 0;
    const int64_t start = chunk_start[rd];
    for (int64_t g = lane; g < R; g += 64) {
      int64_t key = -1;
      double level = 0.0, stdv = 0.0, dwell = 0.0, resid = 0.0;
      const int64_t pos = start + (rev ? R - 1 - g : g);
      if (live && g >= trim && g < R - trim && pos >= 0 && pos < ref_len) {
        int64_t s = events[2 * (r0 + g)], e = events[2 * (r0 + g) + 1];
        s = s < 0 ? 0 : (s > N ? N : s);  // numpy slice clamping, as event_means_kernel
        e = e < 0 ? 0 : (e > N ? N : e);
        if (e > s) {
          key = 2 * pos + (rev ? 1 : 0);
          dwell = (double)(e - s);
          if (e - s <= 128) {  // else: site_long_event_kernel
            event_level_stdv<false>(x + s, e - s, level, stdv);
            resid = level - expected[r0 + g];
          }
        }
      }
      out_key[r0 + g] = key;
      double *dst = out_val + (size_t)(r0 + g) * NCOL;
      dst[0] = level;
      dst[1] = stdv;
      dst[2] = dwell;
      dst[3] = resid;
    }
  }
}

// level, stdv and resid of the counted events of more than 128 samples: one thread per event, the read found by a
// binary search
__global__ __launch_bounds__(NT) void site_long_event_kernel(int64_t n_reads, int64_t total_ref, const double *signal,
                                                             const int64_t *sig_off, const int32_t *events,
                                                             const int64_t *ref_off, const double *expected,
                                                             const int64_t *key, double *out_val) {
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < total_ref; g += (int64_t)gridDim.x * NT) {
    double *dst = out_val + (size_t)g * NCOL;
    if (key[g] < 0 || !(dst[2] > 128.0)) continue;
    const int64_t rd = owner_of(ref_off, n_reads, g);
    const int64_t N = sig_off[rd + 1] - sig_off[rd];
    int64_t s = events[2 * g];
    s = s < 0 ? 0 : (s > N ? N : s);
    double level, stdv;
    event_level_stdv<true>(signal + sig_off[rd] + s, (int64_t)dst[2], level, stdv);
    dst[0] = level;
    dst[1] = stdv;
    dst[3] = level - expected[g];
  }
}

// one wave per key (grid-stride): the count, and per column the mean and the sum of squared deviations of its rows
template <int V>
__global__ __launch_bounds__(NT) void site_moments_kernel(int64_t n_rows, int64_t n_keys, const int64_t *key,
                                                          const double *val, int64_t *out_count, double *out_mean,
                                                          double *out_m2) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t q = (int64_t)blockIdx.x * (NT / 64) + wave; q < n_keys; q += waves) {
    const int64_t lo = lower_bound(key, 0, n_rows, q);
    const int64_t hi = lower_bound(key, lo, n_rows - lo, q + 1);
    const int64_t c = hi - lo;
    const double *v = val + (size_t)lo * V;
    double mean[V], m2[V];
#pragma unroll
    for (int a = 0; a < V; a++) mean[a] = m2[a] = 0.0;
    if (c > 0) {
      for (int64_t i = lane; i < c; i += 64) {
#pragma unroll
        for (int a = 0; a < V; a++) mean[a] += v[(size_t)i * V + a];
      }
      wave_sum_n(mean);
#pragma unroll
      for (int a = 0; a < V; a++) mean[a] = mean[a] / (double)c;
      for (int64_t i = lane; i < c; i += 64) {
#pragma unroll
        for (int a = 0; a < V; a++) {
          const double d = v[(size_t)i * V + a] - mean[a];
          m2[a] += d * d;
        }
      }
      wave_sum_n(m2);
    }
    if (lane == 0) {
      out_count[q] = c;
#pragma unroll
      for (int a = 0; a < V; a++) {
        out_mean[(size_t)q * V + a] = mean[a];
        out_m2[(size_t)q * V + a] = m2[a];
      }
    }
  }
}

}  // namespace

extern "C" int nvk_site_level_rows_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                                       const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                                       const double *expected, const int64_t *chunk_start, const int32_t *reverse,
                                       const int32_t *status, int trim, int64_t ref_len, int64_t *out_key,
                                       double *out_val) {
  const char *what = "nvk_site_level_rows_dev";
  if (!ctx || n_reads < 0 || n_reads > 0x7fffffff || total_ref < 0) {
    nvk_set_error("%s: invalid argument", what);
    return NVK_ERR_INVALID;
  }
  if (trim < 0 || ref_len < 0 || ref_len > ((int64_t)1 << 61)) {
    nvk_set_error("%s: trim %d, ref_len %lld outside the served range (trim >= 0, 0 <= ref_len <= 2^61)", what, trim,
                  (long long)ref_len);
    return NVK_ERR_INVALID;
  }
  if (n_reads == 0) {
    if (total_ref != 0) {
      nvk_set_error("%s: total_ref %lld with no reads", what, (long long)total_ref);
      return NVK_ERR_INVALID;
    }
    return NVK_OK;
  }
  if (!sig_off || !ref_off) {
    nvk_set_error("%s: offsets are NULL", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  int rc;
  if ((rc = nvk_fetch_offsets(ctx, "reference", ref_off, n_reads, off, "total_ref", total_ref))) return rc;
  if ((rc = nvk_fetch_offsets(ctx, "signal", sig_off, n_reads, off))) return rc;
  // (a data array may be NULL only when its offsets end at 0)
  if (off[n_reads] > 0 && !signal) {
    nvk_set_error("%s: signal is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (total_ref == 0) return NVK_OK;
  if (!events || !expected || !chunk_start || !reverse || !out_key || !out_val) {
    nvk_set_error("%s: NULL events, expected, chunk_start, reverse or output", what);
    return NVK_ERR_INVALID;
  }
  {
    TimerScope ts(ctx, NVK_K_SITE);
    hipLaunchKernelGGL(site_rows_kernel, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads, signal,
                       sig_off, events, ref_off, expected, chunk_start, reverse, status, trim, ref_len, out_key,
                       out_val);
    hipLaunchKernelGGL(site_long_event_kernel, dim3(grid_of(total_ref, NT)), dim3(NT), 0, ctx->stream, n_reads,
                       total_ref, signal, sig_off, events, ref_off, expected, (const int64_t *)out_key, out_val);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_site_moments_dev(nvk_ctx *ctx, int64_t n_rows, int64_t n_keys, int n_val, const int64_t *key,
                                    const double *val, int64_t *out_count, double *out_mean, double *out_m2) {
  const char *what = "nvk_site_moments_dev";
  if (!ctx || n_rows < 0 || n_keys < 0 || n_val < 1 || n_val > 8) {
    nvk_set_error("%s: invalid argument (n_rows >= 0, n_keys >= 0, 1 <= n_val <= 8)", what);
    return NVK_ERR_INVALID;
  }
  if (n_keys == 0) return NVK_OK;
  if (!out_count || !out_mean || !out_m2 || (n_rows > 0 && (!key || !val))) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  {
    TimerScope ts(ctx, NVK_K_SITE);
    const dim3 grid(grid_of(n_keys, NT / 64)), block(NT);
#define NVK_SITE_CASE(V)                                                                                            \
  case V:                                                                                                           \
    hipLaunchKernelGGL(site_moments_kernel<V>, grid, block, 0, ctx->stream, n_rows, n_keys, key, val, out_count,    \
                       out_mean, out_m2);                                                                           \
    break;
    switch (n_val) {
      NVK_SITE_CASE(1)
      NVK_SITE_CASE(2)
      NVK_SITE_CASE(3)
      NVK_SITE_CASE(4)
      NVK_SITE_CASE(5)
      NVK_SITE_CASE(6)
      NVK_SITE_CASE(7)
      NVK_SITE_CASE(8)
    }
#undef NVK_SITE_CASE
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
