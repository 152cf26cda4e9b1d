// Per-site modification frequencies over sets of rows (nadavca_amd/phase_mods.py): for every site and every set of
// its rows, the share f^ of the rows that carry the modification, by maximum likelihood over the two-component
// mixture of the rows' log-likelihood ratios, and L(f^) (the contract: include/nadavca_hip.h, nvk_mod_site_solve_dev).
// The estimator is nvk_allele_solve_dev's (kernels_allele.hip): the same t, u, estimate rule and evaluation of L.
//
//   nvk_mod_site_solve_dev   per (site, set): the rows of the set, f^ and L(f^), over the site's rows in the caller's
//                            (stable) order; a set is a mask over the rows' groups, so that "all reads", "haplotype 1",
//                            "haplotype 2" and "tagged" of one site are solved in ONE launch from one pass over d
//
// No floating-point atomics: every sum is a lane's loop over its rows in ascending order followed by wave_sum's
// butterfly, so two runs give the same bits.  Row j of the SITE goes to lane j mod 64 whatever sets it belongs to; a
// row outside a set adds +0.0 to that set's sums.
//
// Work split: ONE WAVE PER SITE (grid-stride), lane l takes rows l, l + 64, ...  The sets are solved SIDE BY SIDE, as
// the alternative bases of a position are in kernels_allele.hip: one sweep over the rows feeds n_sets accumulators and
// their butterflies are interleaved.  What a sweep needs of a row is e = exp(-|d|) with d's sign on it and the row's
// membership bits; both are computed once and stay in registers while the site has at most 64 * CACHE rows, so that
// one exp serves every set and all 54 derivative sweeps.  Beyond that every sweep recomputes them from `val` and
// `group`.  Both paths run the same expressions in the same order (the library is built with -ffp-contract=off) and
// give the same bits.  The 52 bisection sweeps are skipped when no set of the site needs them.  A site of c rows keeps
// min(c, 64) lanes busy; at the coverage of a sequencing run about half the wave idles, the price of sums whose order
// does not depend on the launch.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.16.
#include <math.h>

#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int NT = 256;
constexpr int CACHE = 2;      // rows per lane whose exp(-|d|) stay in registers: sites of up to 64 * CACHE rows
constexpr int BISECT = 52;    // bisection steps on [0, 1]
constexpr int MAX_SETS = 8;

// min(max(d, -clip), clip); -inf gives -clip (and so does a d that is not a number, whose row is in no set)
__device__ __forceinline__ double clipped(double d, double clip) { return d > -clip ? (d < clip ? d : clip) : -clip; }

// exp(-|d|) in [0, 1] carrying the sign of the case: + for d > 0, - otherwise (as kernels_allele.hip)
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

// One site: n rows at v (and g, or NULL).  Every lane of the wave calls it with the same arguments; lane 0 writes the
// site's NS entries.
template <int NS, bool CACHED>
__device__ __forceinline__ void solve_site(int lane, const double *v, const int32_t *g, int64_t n,
                                           const uint32_t (&mask)[NS], double clip, int64_t *out_count,
                                           double *out_fraction, double *out_ll) {
  // bit q: the row is in set q
  auto member = [&](int64_t i, double d) {
    const int grp = g ? g[i] : 0;
    unsigned m = 0;
    if (d == d && grp >= 0 && grp < 32) {
#pragma unroll
      for (int q = 0; q < NS; q++) m |= ((mask[q] >> grp) & 1u) << q;
    }
    return m;
  };
  double se[CACHED ? CACHE : 1];
  unsigned in[CACHED ? CACHE : 1];
  double spos[NS], g0[NS], g1[NS];
  int count[NS];
#pragma unroll
  for (int q = 0; q < NS; q++) {
    spos[q] = g0[q] = g1[q] = 0.0;
    count[q] = 0;
  }

  // first sweep, over d itself: the rows of every set, the sum of its positive values, g(0), g(1)
  auto first = [&](int64_t i, double *keep_e, unsigned *keep_m) {
    const double raw = v[i];
    const unsigned m = member(i, raw);
    const double d = clipped(raw, clip);
    const double s = signed_e(d);
    if (CACHED) {
      *keep_e = s;
      *keep_m = m;
    }
    const double p = d > 0.0 ? d : 0.0, u0 = u_term(0.0, s), u1 = u_term(1.0, s);
#pragma unroll
    for (int q = 0; q < NS; q++) {
      const bool on = (m >> q) & 1u;
      count[q] += on;
      spos[q] += on ? p : 0.0;
      g0[q] += on ? u0 : 0.0;
      g1[q] += on ? u1 : 0.0;
    }
  };
  if (CACHED) {
#pragma unroll
    for (int j = 0; j < CACHE; j++)
      if (lane + 64 * j < n) first(lane + 64 * j, &se[j], &in[j]);
  } else {
    for (int64_t i = lane; i < n; i += 64) first(i, nullptr, nullptr);
  }
  wave_sum_n(spos);
  wave_sum_n(g0);
  wave_sum_n(g1);
#pragma unroll
  for (int q = 0; q < NS; q++) count[q] = wave_sum(count[q]);

  // later sweeps: fn(s, m) per row of the lane, ascending
  auto sweep = [&](auto &&fn) {
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < CACHE; j++)
        if (lane + 64 * j < n) fn(se[j], in[j]);
    } else {
      for (int64_t i = lane; i < n; i += 64) {
        const double raw = v[i];
        fn(signed_e(clipped(raw, clip)), member(i, raw));
      }
    }
  };

  double fhat[NS], lo[NS], hi[NS];
  bool active[NS], any = false;
#pragma unroll
  for (int q = 0; q < NS; q++) {
    fhat[q] = !(g0[q] > 0.0) ? 0.0 : 1.0;
    active[q] = g0[q] > 0.0 && !(g1[q] >= 0.0);
    any = any || active[q];
    lo[q] = 0.0;
    hi[q] = 1.0;
  }
  if (any) {
    for (int it = 0; it < BISECT; it++) {
      double mid[NS], acc[NS];
#pragma unroll
      for (int q = 0; q < NS; q++) {
        mid[q] = (lo[q] + hi[q]) / 2.0;
        acc[q] = 0.0;
      }
      sweep([&](double s, unsigned m) {
#pragma unroll
        for (int q = 0; q < NS; q++)
          if (active[q]) acc[q] += (m >> q) & 1u ? u_term(mid[q], s) : 0.0;
      });
      wave_sum_n(acc);
#pragma unroll
      for (int q = 0; q < NS; q++) {
        if (!active[q]) continue;
        if (acc[q] > 0.0) lo[q] = mid[q]; else hi[q] = mid[q];
      }
    }
#pragma unroll
    for (int q = 0; q < NS; q++)
      if (active[q]) fhat[q] = (lo[q] + hi[q]) / 2.0;
  }

  // L(f^) where f^ > 0
  double lhat[NS];
  any = false;
#pragma unroll
  for (int q = 0; q < NS; q++) {
    lhat[q] = 0.0;
    any = any || fhat[q] > 0.0;
  }
  if (any) {
    sweep([&](double s, unsigned m) {
#pragma unroll
      for (int q = 0; q < NS; q++)
        if (fhat[q] > 0.0) lhat[q] += (m >> q) & 1u ? log_term(fhat[q], s) : 0.0;
    });
    wave_sum_n(lhat);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NS; q++) {
      out_count[q] = count[q];
      out_fraction[q] = fhat[q];
      out_ll[q] = fhat[q] > 0.0 ? spos[q] + lhat[q] : 0.0;
    }
  }
}

// one wave per site (grid-stride)
template <int NS>
__global__ __launch_bounds__(NT) void mod_site_solve_kernel(int64_t n_sites, int64_t n_rows, const int64_t *site_lo,
                                                            const int64_t *site_hi, const double *val,
                                                            const int32_t *group, const uint32_t *set_mask,
                                                            double clip, int64_t *out_count, double *out_fraction,
                                                            double *out_ll) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  uint32_t mask[NS];
#pragma unroll
  for (int q = 0; q < NS; q++) mask[q] = set_mask[q];
  for (int64_t s = (int64_t)blockIdx.x * (NT / 64) + wave; s < n_sites; s += waves) {
    // a range that leaves 0 .. n_rows is cut to it: no read outside `val`
    int64_t lo = uniform64(site_lo[s]), hi = uniform64(site_hi[s]);
    lo = lo < 0 ? 0 : (lo > n_rows ? n_rows : lo);
    hi = hi < lo ? lo : (hi > n_rows ? n_rows : hi);
    const int64_t n = hi - lo;
    int64_t *oc = out_count + (size_t)s * NS;
    double *of = out_fraction + (size_t)s * NS, *ol = out_ll + (size_t)s * NS;
    const double *v = val + lo;
    const int32_t *g = group ? group + lo : nullptr;
    if (n <= 64 * CACHE)
      solve_site<NS, true>(lane, v, g, n, mask, clip, oc, of, ol);
    else
      solve_site<NS, false>(lane, v, g, n, mask, clip, oc, of, ol);
  }
}

}  // namespace

extern "C" int nvk_mod_site_solve_dev(nvk_ctx *ctx, int64_t n_sites, int64_t n_rows, const int64_t *site_lo,
                                      const int64_t *site_hi, const double *val, const int32_t *group, int n_sets,
                                      const uint32_t *set_mask, double clip, int64_t *out_count, double *out_fraction,
                                      double *out_ll) {
  const char *what = "nvk_mod_site_solve_dev";
  if (!ctx || n_sites < 0 || n_rows < 0) {
    nvk_set_error("%s: invalid argument (ctx, n_sites >= 0, n_rows >= 0)", what);
    return NVK_ERR_INVALID;
  }
  if (n_sets < 1 || n_sets > MAX_SETS || !(clip > 0.0) || !(clip < INFINITY)) {
    nvk_set_error("%s: n_sets %d, clip %g outside the served range (1 <= n_sets <= %d, 0 < clip < inf)", what, n_sets,
                  clip, MAX_SETS);
    return NVK_ERR_INVALID;
  }
  if (n_sites == 0) return NVK_OK;
  if (!site_lo || !site_hi || !set_mask || !out_count || !out_fraction || !out_ll || (n_rows > 0 && !val)) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    const dim3 grid(grid_of(n_sites, NT / 64)), block(NT);
#define NVK_MOD_SITE_CASE(NS)                                                                                       \
  case NS:                                                                                                          \
    hipLaunchKernelGGL(mod_site_solve_kernel<NS>, grid, block, 0, ctx->stream, n_sites, n_rows, site_lo, site_hi,   \
                       val, group, set_mask, clip, out_count, out_fraction, out_ll);                                \
    break;
    switch (n_sets) {
      NVK_MOD_SITE_CASE(1)
      NVK_MOD_SITE_CASE(2)
      NVK_MOD_SITE_CASE(3)
      NVK_MOD_SITE_CASE(4)
      NVK_MOD_SITE_CASE(5)
      NVK_MOD_SITE_CASE(6)
      NVK_MOD_SITE_CASE(7)
      NVK_MOD_SITE_CASE(8)
    }
#undef NVK_MOD_SITE_CASE
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
