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
// Work split of the row pass: one wave per read, its lanes over the read's bases, and a second pass for the rare
// event of more than 128 samples (read_rows.h).  A lane reads its event twice, once for the sum and once for the
// squared deviations; the second pass hits the lines the first one fetched, so the pass moves the signal's 8 B per
// sample from memory once, plus 8 B of events and 8 B of expected level in and 40 B out per base.
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
#include "read_rows.h"
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

// the row pass of read_rows.h.  An event of more than 128 samples gets its key and dwell here and level, stdv and
// resid from the second pass.
__global__ __launch_bounds__(NT) void site_rows_kernel(int64_t n_reads, ReadArrays arrays, const int32_t *events,
                                                       const double *expected, int trim, int64_t ref_len,
                                                       int64_t *out_key, double *out_val) {
  for_each_read<int64_t, RV_SIGNAL | RV_STRAND>(arrays, n_reads, [&](const ReadView<int64_t> &v) {
    for_each_base(v, [&](int64_t g) {
      int64_t key = -1;
      double level = 0.0, stdv = 0.0, dwell = 0.0, resid = 0.0;
      const int64_t pos = v.start + (v.rev ? v.R - 1 - g : g);
      if (v.live && counted_base(g, v.R, trim) && pos >= 0 && pos < ref_len) {
        int64_t s, e;
        event_span(events, v.r0 + g, v.N, s, e);
        if (e > s) {
          key = 2 * pos + (v.rev ? 1 : 0);
          dwell = (double)(e - s);
          if (e - s <= 128) {  // else: the second pass
            event_level_stdv<false>(v.x + s, e - s, level, stdv);
            resid = level - expected[v.r0 + g];
          }
        }
      }
      out_key[v.r0 + g] = key;
      double *dst = out_val + (size_t)(v.r0 + g) * NCOL;
      dst[0] = level;
      dst[1] = stdv;
      dst[2] = dwell;
      dst[3] = resid;
    });
  });
}

// the second pass (long_event_kernel): level, stdv and resid of a counted event of more than 128 samples
struct LongSiteLevel {
  const double *expected;
  double *out_val;
  __device__ int64_t length(int64_t g) const {
    const double dwell = out_val[(size_t)g * NCOL + 2];
    return dwell > 128.0 ? (int64_t)dwell : 0;
  }
  __device__ void operator()(int64_t g, const double *xs, int64_t n) const {
    double *dst = out_val + (size_t)g * NCOL;
    double level, stdv;
    event_level_stdv<true>(xs, n, level, stdv);
    dst[0] = level;
    dst[1] = stdv;
    dst[3] = level - expected[g];
  }
};

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
  if (trim < 0 || ref_len < 0 || ref_len > ((int64_t)1 << 61)) {
    nvk_set_error("%s: trim %d, ref_len %lld outside the served range (trim >= 0, 0 <= ref_len <= 2^61)", what, trim,
                  (long long)ref_len);
    return NVK_ERR_INVALID;
  }
  bool nothing;
  int rc = check_read_rows(what, ctx, n_reads, total_ref, ref_off, {{"signal", sig_off, signal}}, &nothing);
  if (rc || nothing) return rc;
  if (!events || !expected || !chunk_start || !reverse || !out_key || !out_val) {
    nvk_set_error("%s: NULL events, expected, chunk_start, reverse or output", what);
    return NVK_ERR_INVALID;
  }
  return nvk_timed(ctx, NVK_K_SITE, [&] {
    const ReadArrays arrays = {ref_off, status, chunk_start, reverse, signal, sig_off};
    hipLaunchKernelGGL(site_rows_kernel, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads, arrays,
                       events, expected, trim, ref_len, out_key, out_val);
    hipLaunchKernelGGL(long_event_kernel, dim3(grid_of(total_ref, NT)), dim3(NT), 0, ctx->stream, n_reads, total_ref,
                       signal, sig_off, events, ref_off, (const int64_t *)out_key, LongSiteLevel{expected, out_val});
  });
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
  return nvk_timed(ctx, NVK_K_SITE, [&] {
    dispatch_int<1, 8>(n_val, [&](auto v) {
      hipLaunchKernelGGL(site_moments_kernel<decltype(v)::value>, dim3(grid_of(n_keys, NT / 64)), dim3(NT), 0,
                         ctx->stream, n_rows, n_keys, key, val, out_count, out_mean, out_m2);
    });
  });
}
