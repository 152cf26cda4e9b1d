// The two-component mixture estimator of the per-site solvers (allele_solve_kernel: one problem per alternative base;
// mod_site_solve_kernel: one problem per set of rows): the share f^ in [0, 1] that maximises
//     L(f) = sum_i t(f, d_i),   t(f, d) = log(f e^d + 1 - f)
// over the log-likelihood ratios d_i of the rows of one problem, and L(f^).
//
// Work split: ONE WAVE PER SITE, lane l takes rows l, l + 64, ...  The NC problems of a site are solved SIDE BY SIDE:
// one sweep over the rows feeds NC accumulators and their butterflies are interleaved (wave_sum_n), so that one
// shuffle's latency hides behind the others'.  What a sweep needs of a value d is e = exp(-|d|) and the sign of d,
// never exp(d) for a positive d (d reaches hundreds of nats): e is computed once and kept with d's sign on it (-0.0
// tells d = -inf from a large positive d).  The caller keeps it in registers while the site has at most
// 64 * MIX_CACHE rows and recomputes it in every sweep beyond that; both ways run the same expressions in the same
// order (the library is built with -ffp-contract=off) and give the same bits.  A row outside a problem adds +0.0 to
// that problem's sums.  L is concave, so g = dL/df decides: g(0) <= 0 means f^ = 0, g(1) >= 0 means f^ = 1, else g
// has its root inside and 52 bisection sweeps find it; they are skipped when no problem of the site needs them, which
// is most sites.  No floating-point atomics: every sum is a lane's loop over its rows in ascending order followed by a
// butterfly over the wave, so two runs give the same bits.
#pragma once
#include <math.h>

#include "wave.h"

constexpr int MIX_CACHE = 2;    // rows per lane whose exp(-|d|) stay in registers: sites of up to 64 * MIX_CACHE rows
constexpr int MIX_BISECT = 52;  // bisection steps on [0, 1]

// a row's log-likelihood ratio as the site kernels take it (the mixtures here, the phase kernels' evidence):
// min(max(d, -clip), clip); -inf and a d that is not a number give -clip
__device__ __forceinline__ double clipped(double d, double clip) { return d > -clip ? (d < clip ? d : clip) : -clip; }

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

// NC problems over the rows of one site.  Every lane of the wave calls it with the same site; the results are in every
// lane: fhat[c], spos[c] = the sum of the problem's positive d, and lhat[c] = sum log_term(f^, .) where f^ > 0 (else
// 0), so that L(f^) = spos + lhat.  The caller supplies the rows:
//   first(fn)   fn(row) for each row of the lane, ascending, as it reads d; it may keep what `again` needs and add up
//               sums of its own
//   again(fn)   the same rows once more, from registers or from memory
//   row.se(c)   the signed e of problem c;  row.in(c): the row belongs to problem c;  row.d(c): d itself, under
//               `first` only
template <int NC, class First, class Again>
__device__ __forceinline__ void mix_mle(First &&first, Again &&again, double (&fhat)[NC], double (&spos)[NC],
                                        double (&lhat)[NC]) {
  double g0[NC], g1[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) spos[c] = g0[c] = g1[c] = 0.0;
  // first sweep, over d itself: the sum of the positive d, g(0), g(1)
  first([&](const auto &row) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const bool on = row.in(c);
      const double d = row.d(c), s = row.se(c);
      spos[c] += on ? (d > 0.0 ? d : 0.0) : 0.0;
      g0[c] += on ? u_term(0.0, s) : 0.0;
      g1[c] += on ? u_term(1.0, s) : 0.0;
    }
  });
  wave_sum_n(spos);
  wave_sum_n(g0);
  wave_sum_n(g1);

  double lo[NC], hi[NC];
  bool active[NC], any = false;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    fhat[c] = !(g0[c] > 0.0) ? 0.0 : 1.0;
    active[c] = g0[c] > 0.0 && !(g1[c] >= 0.0);
    any = any || active[c];
    lo[c] = 0.0;
    hi[c] = 1.0;
  }
  if (any) {
    for (int it = 0; it < MIX_BISECT; it++) {
      double mid[NC], acc[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) {
        mid[c] = (lo[c] + hi[c]) / 2.0;
        acc[c] = 0.0;
      }
      again([&](const auto &row) {
#pragma unroll
        for (int c = 0; c < NC; c++)
          if (active[c]) acc[c] += row.in(c) ? u_term(mid[c], row.se(c)) : 0.0;
      });
      wave_sum_n(acc);
#pragma unroll
      for (int c = 0; c < NC; c++) {
        if (!active[c]) continue;
        if (acc[c] > 0.0) lo[c] = mid[c]; else hi[c] = mid[c];
      }
    }
#pragma unroll
    for (int c = 0; c < NC; c++)
      if (active[c]) fhat[c] = (lo[c] + hi[c]) / 2.0;
  }

  // L(f^) where f^ > 0
  any = false;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    lhat[c] = 0.0;
    any = any || fhat[c] > 0.0;
  }
  if (any) {
    again([&](const auto &row) {
#pragma unroll
      for (int c = 0; c < NC; c++)
        if (fhat[c] > 0.0) lhat[c] += row.in(c) ? log_term(fhat[c], row.se(c)) : 0.0;
    });
    wave_sum_n(lhat);
  }
}
