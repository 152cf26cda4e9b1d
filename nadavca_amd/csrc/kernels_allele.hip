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
// Work split of the row pass: one wave per read, its lanes over the read's rows (read_rows.h); the read's shift is
// wave-uniform with the rest of its view.  The pass moves 8 * alphabet bytes in and 8 * alphabet + 8 out per row.
//
// Work split of the solve: ONE WAVE PER POSITION (grid-stride).  The position's rows are contiguous after the sort;
// their range comes from two wave-uniform binary searches over the keys, lane l takes rows l, l + 64, ...  The
// alphabet - 1 alternative bases are the problems that mix_mle.h solves side by side; what is here is the map from
// problems to columns, the two sums that only this operator reports (L(1) and the logarithms of L(1/2)) and the
// outputs.  A position of coverage c keeps min(c, 64) lanes busy; at the coverage of a sequencing run (tens of
// reads) about half the wave idles, which is the price of sums whose order does not depend on the launch.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.4.
#include <math.h>

#include <vector>

#include "mix_mle.h"
#include "nvk_internal.h"
#include "read_rows.h"
#include "wave.h"

namespace {

constexpr int NT = 256;

// the row pass of read_rows.h
__global__ __launch_bounds__(NT) void allele_rows_kernel(int64_t n_reads, ReadArrays arrays, int alpha,
                                                         const double *ll, const int32_t *reference,
                                                         double event_length, int64_t ref_len, int64_t *out_key,
                                                         double *out_val) {
  for_each_read<int64_t, RV_STRAND>(arrays, n_reads, [&](const ReadView<int64_t> &v) {
    bool live = v.live;
    double shift = 0.0;
    if (live) {
      // shift = likelihoods[0][reference[0]], the read's total without a substitution (as consensus_kernel)
      const int c0 = reference[v.r0];
      live = c0 >= 0 && c0 < alpha;
      if (live) {
        shift = ll[(size_t)v.r0 * alpha + c0];
        live = isfinite(shift);
      }
    }
    for_each_base(v, [&](int64_t g) {
      // reverse strand: complement the columns and flip the rows (as consensus_kernel)
      const int64_t pos = v.start + (v.rev ? v.R - 1 - g : g);
      const bool ok = live && pos >= 0 && pos < ref_len;
      out_key[v.r0 + g] = ok ? pos : -1;
      const double *src = ll + (size_t)(v.r0 + g) * alpha;
      double *dst = out_val + (size_t)(v.r0 + g) * alpha;
      for (int b = 0; b < alpha; b++) dst[v.rev ? alpha - 1 - b : b] = ok ? (src[b] - shift) / event_length : 0.0;
    });
  });
}

// a row of a position as mix_mle sees it: problem a has its own value, and every row belongs to every problem
struct AlleleRow {
  const double *dv, *sv;
  __device__ double d(int a) const { return dv[a]; }
  __device__ double se(int a) const { return sv[a]; }
  __device__ bool in(int) const { return true; }
};

// One position: n rows of A values at v, reference base r in 0 .. A-1; out_*: the position's A entries.  Every lane of
// the wave calls it with the same arguments; lane 0 writes.
template <int A, bool CACHED>
__device__ __forceinline__ void solve_position(int lane, const double *v, int64_t n, int r, double *out_fraction,
                                               double *out_lrt, double *out_half, double *out_full) {
  constexpr int NA = A - 1;
  auto column = [&](int a) { return a + (a >= r ? 1 : 0); };   // the a-th base other than r
  double se[CACHED ? MIX_CACHE : 1][NA];
  double full[NA], half[NA];
#pragma unroll
  for (int a = 0; a < NA; a++) full[a] = half[a] = 0.0;

  // the first sweep also takes sum d and the logarithms of L(1/2)
  auto first = [&](auto &&fn) {
    auto at = [&](int64_t i, double *keep) {
      double d[NA], s[NA];
#pragma unroll
      for (int a = 0; a < NA; a++) {
        d[a] = v[(size_t)i * A + column(a)];
        s[a] = signed_e(d[a]);
        if (CACHED) keep[a] = s[a];
        full[a] += d[a];
        half[a] += log_term(0.5, s[a]);
      }
      fn(AlleleRow{d, s});
    };
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < MIX_CACHE; j++)
        if (lane + 64 * j < n) at(lane + 64 * j, se[j]);
    } else {
      for (int64_t i = lane; i < n; i += 64) at(i, nullptr);
    }
  };
  auto again = [&](auto &&fn) {
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < MIX_CACHE; j++)
        if (lane + 64 * j < n) fn(AlleleRow{nullptr, se[j]});
    } else {
      for (int64_t i = lane; i < n; i += 64) {
        double s[NA];
#pragma unroll
        for (int a = 0; a < NA; a++) s[a] = signed_e(v[(size_t)i * A + column(a)]);
        fn(AlleleRow{nullptr, s});
      }
    }
  };
  double fhat[NA], spos[NA], lhat[NA];
  mix_mle<NA>(first, again, fhat, spos, lhat);
  wave_sum_n(full);
  wave_sum_n(half);
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
    if (n <= 64 * MIX_CACHE)
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
  if (ref_len < 0) {
    nvk_set_error("%s: invalid argument", what);
    return NVK_ERR_INVALID;
  }
  if (alphabet < 2 || alphabet > 8 || !(event_length > 0.0) || !(event_length < INFINITY)) {
    nvk_set_error("%s: alphabet %d, event_length %g outside the served range (2 <= alphabet <= 8, 0 < event_length "
                  "< inf)", what, alphabet, event_length);
    return NVK_ERR_INVALID;
  }
  bool nothing;
  int rc = check_read_rows(what, ctx, n_reads, total_ref, ref_off, {}, &nothing);
  if (rc || nothing) return rc;
  if (!ll || !reference || !chunk_start || !reverse || !out_key || !out_val) {
    nvk_set_error("%s: NULL ll, reference, chunk_start, reverse or output", what);
    return NVK_ERR_INVALID;
  }
  return nvk_timed(ctx, NVK_K_ALLELE, [&] {
    const ReadArrays arrays = {ref_off, status, chunk_start, reverse};
    hipLaunchKernelGGL(allele_rows_kernel, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads, arrays,
                       alphabet, ll, reference, event_length, ref_len, out_key, out_val);
  });
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
  return nvk_timed(ctx, NVK_K_ALLELE, [&] {
    dispatch_int<2, 8>(alphabet, [&](auto a) {
      hipLaunchKernelGGL(allele_solve_kernel<decltype(a)::value>, dim3(grid_of(ref_len, NT / 64)), dim3(NT), 0,
                         ctx->stream, n_rows, ref_len, key, val, ref_codes, out_fraction, out_lrt, out_ll_half,
                         out_ll_full, out_coverage);
    });
  });
}
