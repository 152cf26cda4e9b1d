// Per-site modification frequencies over sets of rows (nadavca_amd/phase_mods.py): for every site and every set of
// its rows, the share f^ of the rows that carry the modification, by maximum likelihood over the two-component
// mixture of the rows' log-likelihood ratios, and L(f^) (the contract: include/nadavca_hip.h, nvk_mod_site_solve_dev).
// The estimator is mix_mle.h's, one problem per set.
//
//   nvk_mod_site_solve_dev   per (site, set): the rows of the set, f^ and L(f^), over the site's rows in the caller's
//                            (stable) order; a set is a mask over the rows' groups, so that "all reads", "haplotype 1",
//                            "haplotype 2" and "tagged" of one site are solved in ONE launch from one pass over d
//
// Work split: ONE WAVE PER SITE (grid-stride), lane l takes rows l, l + 64, ...: row j of the SITE goes to lane
// j mod 64 whatever sets it belongs to, and a row outside a set adds +0.0 to that set's sums.  What is here is what a
// row is: its value clipped, and its membership bits.  Both are computed once and stay in registers while the site
// has at most 64 * MIX_CACHE rows, so that one exp serves every set and all 54 derivative sweeps; beyond that every
// sweep recomputes them from `val` and `group`.  A site of c rows keeps min(c, 64) lanes busy; at the coverage of a
// sequencing run about half the wave idles, the price of sums whose order does not depend on the launch.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.16.
#include <math.h>

#include "mix_mle.h"
#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_SETS = 8;

// a row of a site as mix_mle sees it: one value for every set, and bit q of m says whether the row is in set q
struct SiteRow {
  double dv, sv;
  unsigned m;
  __device__ double d(int) const { return dv; }
  __device__ double se(int) const { return sv; }
  __device__ bool in(int q) const { return (m >> q) & 1u; }
};

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
  double se[CACHED ? MIX_CACHE : 1];
  unsigned in[CACHED ? MIX_CACHE : 1];
  int count[NS];
#pragma unroll
  for (int q = 0; q < NS; q++) count[q] = 0;

  // the first sweep also counts the rows of every set
  auto first = [&](auto &&fn) {
    auto at = [&](int64_t i, double *keep_e, unsigned *keep_m) {
      const double raw = v[i];
      const unsigned m = member(i, raw);
      const double d = clipped(raw, clip);
      const double s = signed_e(d);
      if (CACHED) {
        *keep_e = s;
        *keep_m = m;
      }
#pragma unroll
      for (int q = 0; q < NS; q++) count[q] += (m >> q) & 1u;
      fn(SiteRow{d, s, m});
    };
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < MIX_CACHE; j++)
        if (lane + 64 * j < n) at(lane + 64 * j, &se[j], &in[j]);
    } else {
      for (int64_t i = lane; i < n; i += 64) at(i, nullptr, nullptr);
    }
  };
  auto again = [&](auto &&fn) {
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < MIX_CACHE; j++)
        if (lane + 64 * j < n) fn(SiteRow{0.0, se[j], in[j]});
    } else {
      for (int64_t i = lane; i < n; i += 64) {
        const double raw = v[i];
        fn(SiteRow{0.0, signed_e(clipped(raw, clip)), member(i, raw)});
      }
    }
  };
  double fhat[NS], spos[NS], lhat[NS];
  mix_mle<NS>(first, again, fhat, spos, lhat);
#pragma unroll
  for (int q = 0; q < NS; q++) count[q] = wave_sum(count[q]);
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
    if (n <= 64 * MIX_CACHE)
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
  return nvk_timed(ctx, NVK_K_ALLELE, [&] {
    dispatch_int<1, MAX_SETS>(n_sets, [&](auto ns) {
      hipLaunchKernelGGL(mod_site_solve_kernel<decltype(ns)::value>, dim3(grid_of(n_sites, NT / 64)), dim3(NT), 0,
                         ctx->stream, n_sites, n_rows, site_lo, site_hi, val, group, set_mask, clip, out_count,
                         out_fraction, out_ll);
    });
  });
}
