// Per-site allele mixtures (nadavca_amd/allele_fractions.py): for every reference position and every base other than
// the reference's, the share of the covering reads that carry it, by maximum likelihood over a two-component mixture
// of the reads' own log-likelihood ratios (the contract: include/nadavca_hip.h, nvk_allele_rows_dev).
//
//   nvk_allele_rows_dev    per (read, base position): its global position as a sort key and its row of normalised,
//                          strand-corrected log-likelihood ratios d (what consensus_kernel adds into its sums)
//   nvk_allele_solve_dev   per position: coverage, and per alternative base the fraction f^ that maximises
//                          L(f) = sum_i t(f, d_i), 2 L(f^), L(1/2) and L(1), over the position's rows in stable key
//                          order (the caller sorts and gathers: plumbing)
//
// No floating-point atomics: every sum is a lane's loop over its rows in ascending order followed by a butterfly over
// the wave, so two runs give the same bits.
//
// Work split of the row pass: ONE WAVE PER READ, lanes over its rows; offsets, status, strand and shift are
// wave-uniform, as in kmer_event_kernel.  The pass moves 8 * alphabet bytes in and 8 * alphabet + 8 out per row.
//
// Work split of the solve: ONE WAVE PER POSITION (grid-stride).  The position's rows are contiguous after the sort;
// their range comes from two wave-uniform binary searches over the keys, lane l takes rows l, l + 64, ...  The
// alphabet - 1 alternative bases are solved SIDE BY SIDE: one sweep over the rows feeds alphabet - 1 accumulators and
// their butterflies are interleaved, so that one shuffle's latency hides behind the others'.  What a sweep needs of
// a value d is e = exp(-|d|) and the sign of d, never exp(d) for a positive d (d reaches hundreds of nats): e is
// computed once, kept with d's sign on it (-0.0 tells d = -inf from a large positive d), and stays in registers
// while the position has at most 64 * CACHE rows; beyond that every sweep recomputes it from `val`.  Both paths run
// the same expressions in the same order (the library is built with -ffp-contract=off) and give the same bits.
// Most (position, base) pairs end after the first sweep: g(0) <= 0 means f^ = 0, and the 52 bisection sweeps are
// skipped when no base of the position needs them.  A position of coverage c keeps min(c, 64) lanes busy; at the
// coverage of a sequencing run (tens of reads) about half the wave idles, which is the price of sums whose order
// does not depend on the launch.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.4.
#include <math.h>

#include <vector>

#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int NT = 256;
constexpr int CACHE = 2;      // rows per lane whose exp(-|d|) stay in registers: positions of up to 64 * CACHE rows
constexpr int BISECT = 52;    // bisection steps on [0, 1]

// one wave per read (grid-stride), its lanes over the read's rows
__global__ __launch_bounds__(NT) void allele_rows_kernel(int64_t n_reads, int alpha, const double *ll,
                                                         const int32_t *reference, const int64_t *ref_off,
                                                         const int64_t *chunk_start, const int32_t *reverse,
                                                         const int32_t *status, double event_length, int64_t ref_len,
                                                         int64_t *out_key, double *out_val) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t rd = (int64_t)blockIdx.x * (NT / 64) + wave; rd < n_reads; rd += waves) {
    const int64_t r0 = ref_off[rd];
    const int64_t R = ref_off[rd + 1] - r0;
    if (R <= 0) continue;
    bool live = !status || status[rd] == NVK_READ_OK;
    double shift = 0.0;
    if (live) {
      // shift = likelihoods[0][reference[0]], the read's total without a substitution (as consensus_kernel)
      const int c0 = reference[r0];
      live = c0 >= 0 && c0 < alpha;
      if (live) {
        shift = ll[(size_t)r0 * alpha + c0];
        live = isfinite(shift);
      }
    }
    const bool rev = reverse[rd] != 0;
    const int64_t start = chunk_start[rd];
    for (int64_t g = lane; g < R; g += 64) {
      // reverse strand: complement the columns and flip the rows (as consensus_kernel)
      const int64_t pos = start + (rev ? R - 1 - g : g);
      const bool ok = live && pos >= 0 && pos < ref_len;
      out_key[r0 + g] = ok ? pos : -1;
      const double *src = ll + (size_t)(r0 + g) * alpha;
      double *dst = out_val + (size_t)(r0 + g) * alpha;
      for (int b = 0; b < alpha; b++) dst[rev ? alpha - 1 - b : b] = ok ? (src[b] - shift) / event_length : 0.0;
    }
  }
}

// exp(-|d|) in [0, 1] carrying the sign of the case: + for d > 0, - otherwise (-0.0 for d = -inf)
__device__ __forceinline__ double signed_e(double d) { return copysign(exp(-fabs(d)), d > 0.0 ? 1.0 : -1.0); }

// u(f, d) = d/df t(f, d):  (1 - e) / (e (1 - f) + f) for d > 0,  (e - 1) / (1 + f (e - 1)) otherwise
__device__ __forceinline__ double u_term(double f, double se) {
  const double e = fabs(se);
  const bool pos = !signbit(se);
  const double num = pos ? 1.0 - e : e - 1.0;
  const double den = pos ? e * (1.0 - f) + f : 1.0 + f * (e - 1.0);
  return num / den;
}

// t(f, d) without the summand d of the case d > 0:  log(f + (1 - f) e) for d > 0,  log((1 - f) + f e) otherwise
__device__ __forceinline__ double log_term(double f, double se) {
  const double e = fabs(se);
  return log(!signbit(se) ? f + (1.0 - f) * e : (1.0 - f) + f * e);
}

// One position: n rows of A values at v, reference base r in 0 .. A-1; out_*: the position's A entries.  Every lane of
// the wave calls it with the same arguments; lane 0 writes.
template <int A, bool CACHED>
__device__ __forceinline__ void solve_position(int lane, const double *v, int64_t n, int r, double *out_fraction,
                                               double *out_lrt, double *out_half, double *out_full) {
  constexpr int NA = A - 1;
  auto column = [&](int a) { return a + (a >= r ? 1 : 0); };   // the a-th base other than r
  double se[CACHED ? CACHE : 1][NA];
  double full[NA], spos[NA], g0[NA], g1[NA], half[NA];
#pragma unroll
  for (int a = 0; a < NA; a++) full[a] = spos[a] = g0[a] = g1[a] = half[a] = 0.0;

  // first sweep, over d itself: sum d, sum of the positive d, g(0), g(1), the logarithms of L(1/2)
  auto first = [&](int64_t i, double *keep) {
#pragma unroll
    for (int a = 0; a < NA; a++) {
      const double d = v[(size_t)i * A + column(a)];
      const double s = signed_e(d);
      if (CACHED) keep[a] = s;
      full[a] += d;
      spos[a] += d > 0.0 ? d : 0.0;
      g0[a] += u_term(0.0, s);
      g1[a] += u_term(1.0, s);
      half[a] += log_term(0.5, s);
    }
  };
  if (CACHED) {
#pragma unroll
    for (int j = 0; j < CACHE; j++)
      if (lane + 64 * j < n) first(lane + 64 * j, se[j]);
  } else {
    for (int64_t i = lane; i < n; i += 64) first(i, nullptr);
  }
  wave_sum_n(full);
  wave_sum_n(spos);
  wave_sum_n(g0);
  wave_sum_n(g1);
  wave_sum_n(half);

  // later sweeps: fn(s[NA]) per row of the lane, ascending
  auto sweep = [&](auto &&fn) {
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < CACHE; j++)
        if (lane + 64 * j < n) fn(se[j]);
    } else {
      for (int64_t i = lane; i < n; i += 64) {
        double s[NA];
#pragma unroll
        for (int a = 0; a < NA; a++) s[a] = signed_e(v[(size_t)i * A + column(a)]);
        fn(s);
      }
    }
  };

  double fhat[NA], lo[NA], hi[NA];
  bool active[NA], any = false;
#pragma unroll
  for (int a = 0; a < NA; a++) {
    fhat[a] = !(g0[a] > 0.0) ? 0.0 : 1.0;
    active[a] = g0[a] > 0.0 && !(g1[a] >= 0.0);
    any = any || active[a];
    lo[a] = 0.0;
    hi[a] = 1.0;
  }
  if (any) {
    for (int it = 0; it < BISECT; it++) {
      double m[NA], acc[NA];
#pragma unroll
      for (int a = 0; a < NA; a++) {
        m[a] = (lo[a] + hi[a]) / 2.0;
        acc[a] = 0.0;
      }
      sweep([&](const double *s) {
#pragma unroll
        for (int a = 0; a < NA; a++)
          if (active[a]) acc[a] += u_term(m[a], s[a]);
      });
      wave_sum_n(acc);
#pragma unroll
      for (int a = 0; a < NA; a++) {
        if (!active[a]) continue;
        if (acc[a] > 0.0) lo[a] = m[a]; else hi[a] = m[a];
      }
    }
#pragma unroll
    for (int a = 0; a < NA; a++)
      if (active[a]) fhat[a] = (lo[a] + hi[a]) / 2.0;
  }

  // L(f^) where f^ > 0
  double lhat[NA];
  any = false;
#pragma unroll
  for (int a = 0; a < NA; a++) {
    lhat[a] = 0.0;
    any = any || fhat[a] > 0.0;
  }
  if (any) {
    sweep([&](const double *s) {
#pragma unroll
      for (int a = 0; a < NA; a++)
        if (fhat[a] > 0.0) lhat[a] += log_term(fhat[a], s[a]);
    });
    wave_sum_n(lhat);
  }
  if (lane == 0) {
    out_fraction[r] = out_lrt[r] = out_half[r] = out_full[r] = 0.0;
#pragma unroll
    for (int a = 0; a < NA; a++) {
      const int c = column(a);
      out_fraction[c] = fhat[a];
      out_lrt[c] = fhat[a] > 0.0 ? 2.0 * (spos[a] + lhat[a]) : 0.0;
      out_half[c] = spos[a] + half[a];
      out_full[c] = full[a];
    }
  }
}

// one wave per position (grid-stride)
template <int A>
__global__ __launch_bounds__(NT) void allele_solve_kernel(int64_t n_rows, int64_t ref_len, const int64_t *key,
                                                          const double *val, const int32_t *ref_codes,
                                                          double *out_fraction, double *out_lrt, double *out_half,
                                                          double *out_full, int64_t *out_coverage) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t P = (int64_t)blockIdx.x * (NT / 64) + wave; P < ref_len; P += waves) {
    const int64_t lo = lower_bound(key, 0, n_rows, P);
    const int64_t hi = lower_bound(key, lo, n_rows - lo, P + 1);
    const int64_t n = hi - lo;
    const int r = ref_codes[P];
    double *of = out_fraction + (size_t)P * A, *ol = out_lrt + (size_t)P * A;
    double *oh = out_half + (size_t)P * A, *ou = out_full + (size_t)P * A;
    if (lane == 0) out_coverage[P] = n;
    if (n == 0 || r < 0 || r >= A) {
      if (lane < A) of[lane] = ol[lane] = oh[lane] = ou[lane] = 0.0;
      continue;
    }
    const double *v = val + (size_t)lo * A;
    if (n <= 64 * CACHE)
      solve_position<A, true>(lane, v, n, r, of, ol, oh, ou);
    else
      solve_position<A, false>(lane, v, n, r, of, ol, oh, ou);
  }
}

}  // namespace

extern "C" int nvk_allele_rows_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, int alphabet, const double *ll,
                                   const int32_t *reference, const int64_t *ref_off, const int64_t *chunk_start,
                                   const int32_t *reverse, const int32_t *status, double event_length,
                                   int64_t ref_len, int64_t *out_key, double *out_val) {
  const char *what = "nvk_allele_rows_dev";
  if (!ctx || n_reads < 0 || n_reads > 0x7fffffff || total_ref < 0 || ref_len < 0) {
    nvk_set_error("%s: invalid argument", what);
    return NVK_ERR_INVALID;
  }
  if (alphabet < 2 || alphabet > 8 || !(event_length > 0.0) || !(event_length < INFINITY)) {
    nvk_set_error("%s: alphabet %d, event_length %g outside the served range (2 <= alphabet <= 8, 0 < event_length "
                  "< inf)", what, alphabet, event_length);
    return NVK_ERR_INVALID;
  }
  if (n_reads == 0) {
    if (total_ref != 0) {
      nvk_set_error("%s: total_ref %lld with no reads", what, (long long)total_ref);
      return NVK_ERR_INVALID;
    }
    return NVK_OK;
  }
  if (!ref_off) {
    nvk_set_error("%s: offsets are NULL", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  int rc;
  if ((rc = nvk_fetch_offsets(ctx, "reference", ref_off, n_reads, off, "total_ref", total_ref))) return rc;
  if (total_ref == 0) return NVK_OK;
  if (!ll || !reference || !chunk_start || !reverse || !out_key || !out_val) {
    nvk_set_error("%s: NULL ll, reference, chunk_start, reverse or output", what);
    return NVK_ERR_INVALID;
  }
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    hipLaunchKernelGGL(allele_rows_kernel, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads,
                       alphabet, ll, reference, ref_off, chunk_start, reverse, status, event_length, ref_len, out_key,
                       out_val);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_allele_solve_dev(nvk_ctx *ctx, int64_t n_rows, int64_t ref_len, int alphabet, const int64_t *key,
                                    const double *val, const int32_t *ref_codes, double *out_fraction,
                                    double *out_lrt, double *out_ll_half, double *out_ll_full,
                                    int64_t *out_coverage) {
  const char *what = "nvk_allele_solve_dev";
  if (!ctx || n_rows < 0 || ref_len < 0 || alphabet < 2 || alphabet > 8) {
    nvk_set_error("%s: invalid argument (n_rows >= 0, ref_len >= 0, 2 <= alphabet <= 8)", what);
    return NVK_ERR_INVALID;
  }
  if (ref_len == 0) return NVK_OK;
  if (!ref_codes || !out_fraction || !out_lrt || !out_ll_half || !out_ll_full || !out_coverage ||
      (n_rows > 0 && (!key || !val))) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    const dim3 grid(grid_of(ref_len, NT / 64)), block(NT);
#define NVK_ALLELE_CASE(A)                                                                                          \
  case A:                                                                                                           \
    hipLaunchKernelGGL(allele_solve_kernel<A>, grid, block, 0, ctx->stream, n_rows, ref_len, key, val, ref_codes,   \
                       out_fraction, out_lrt, out_ll_half, out_ll_full, out_coverage);                              \
    break;
    switch (alphabet) {
      NVK_ALLELE_CASE(2)
      NVK_ALLELE_CASE(3)
      NVK_ALLELE_CASE(4)
      NVK_ALLELE_CASE(5)
      NVK_ALLELE_CASE(6)
      NVK_ALLELE_CASE(7)
      NVK_ALLELE_CASE(8)
    }
#undef NVK_ALLELE_CASE
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
