// Per-site rank tests between two samples (nadavca_amd/site_ranks.py): for every listed (position, strand) the exact
// integers of the two-sample Kolmogorov-Smirnov and Mann-Whitney statistics over the two pile-ups of one event column,
// and the exact two-sided p-value of the KS statistic (the contract: include/nadavca_hip.h, nvk_site_rank_tests_dev).
//
// Work split: ONE WAVE PER LISTED SITE (grid-stride), so the launch scales with the sites tested and not with the
// genome.  The two runs of the site come from wave-uniform binary searches on the sorted keys.
//
//   integer statistics   lanes stride over the elements of A and then of B.  Every element binary-searches both runs for
//                        the numbers of values below it and not above it; from those it has the two KS numerators at
//                        its value, its share of 2 U and, if it is the first element of its tie group (in A, or in B
//                        with no equal value in A), the group's t^3 - t.  Maximum and sums are integer butterflies:
//                        no order dependence.
//   exact KS p-value     the lattice recurrence V(a, b) = (V(a-1, b) a + V(a, b-1) b) / (a + b) with V = 1 where
//                        |a P - b p| >= h.  The SMALLER sample's index a (p + 1 <= 256 values) lies on the lanes, four
//                        contiguous a per lane in registers; the sweep goes over the anti-diagonals s = a + b =
//                        1 .. p + P, and the one cross-lane value per step is the left lane's last register (wave_ror:1;
//                        lane 0 takes 0.0).  h and the p-value are symmetric under swapping the samples, and so are the
//                        bits: the two products change places in a sum of two.
//
// At sequencing coverage (10 .. 20 per strand) three to six lanes of the wave work; DESIGN.md 4.6 has the time this
// costs.  Resources on gfx950: no LDS, no scratch, no atomics; the register counts are in DESIGN.md 4.6.
#include <math.h>

#include "site_runs.h"

namespace {

constexpr int NT = 256;
constexpr int PER_LANE = 4;                 // contiguous indices of the smaller sample per lane
constexpr int64_t MAX_SMALL = 64 * PER_LANE - 1;  // 255: the largest smaller sample the recurrence serves

// the number of v[0 .. n) below x / not above x; v ascending
__device__ __forceinline__ int64_t count_lt(const double *v, int64_t n, double x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t count_le(const double *v, int64_t n, double x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t wave_max64(int64_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor((long long)v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// V(p, P) of the recurrence above, in every lane; 1 <= p <= MAX_SMALL, p <= P, h >= 0
__device__ __forceinline__ double ks_exact_p(int lane, int64_t p, int64_t P, int64_t h) {
  double v[PER_LANE], fa[PER_LANE];
  int64_t d[PER_LANE];  // a P - b p of the register's cell on the current anti-diagonal
#pragma unroll
  for (int r = 0; r < PER_LANE; r++) {
    const int a = PER_LANE * lane + r;
    v[r] = 0.0;
    fa[r] = (double)a;
    d[r] = (int64_t)a * (P + p);  // b = s - a with s = 0
  }
  if (lane == 0) v[0] = h <= 0 ? 1.0 : 0.0;  // V(0, 0)
  const int64_t steps = p + P;
  for (int64_t s = 1; s <= steps; s++) {
    const double fs = (double)s;
    double left = dpp_ror1(v[PER_LANE - 1]);
    if (lane == 0) left = 0.0;
    double nv[PER_LANE];
#pragma unroll
    for (int r = 0; r < PER_LANE; r++) {
      const int64_t a = PER_LANE * lane + r;
      const int64_t b = s - a;
      d[r] -= p;
      const double up = r == 0 ? left : v[r - 1];  // V(a - 1, b)
      const int64_t ad = d[r] < 0 ? -d[r] : d[r];
      double x = (up * fa[r] + v[r] * (double)b) / fs;
      if (ad >= h) x = 1.0;
      nv[r] = (b >= 0 && b <= P && a <= p) ? x : 0.0;
    }
#pragma unroll
    for (int r = 0; r < PER_LANE; r++) v[r] = nv[r];
  }
  double mine = 0.0;
#pragma unroll
  for (int r = 0; r < PER_LANE; r++)
    if (PER_LANE * lane + r == p) mine = v[r];
  return __shfl(mine, (int)(p / PER_LANE), 64);
}

__global__ __launch_bounds__(NT) void site_rank_tests_kernel(int64_t n_rows_a, const int64_t *key_a,
                                                             const double *val_a, int64_t n_rows_b,
                                                             const int64_t *key_b, const double *val_b,
                                                             int64_t n_sites, const int64_t *site_key,
                                                             int64_t exact_cells, int64_t *out_n_a, int64_t *out_n_b,
                                                             int64_t *out_ks_plus, int64_t *out_ks_minus,
                                                             int64_t *out_u2, int64_t *out_tie, double *out_ks_p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wave; t < n_sites; t += waves) {
    const auto [la, n, lb, m] = site_runs(key_a, n_rows_a, key_b, n_rows_b, site_key[t]);
    const double *A = val_a + la, *B = val_b + lb;
    int64_t ks_plus = 0, ks_minus = 0, u2 = 0, tie = 0;
    double ks_p = NAN;
    if (n > 0 && m > 0) {
      for (int64_t i = lane; i < n + m; i += 64) {
        const bool in_a = i < n;
        const int64_t own = in_a ? i : i - n;
        const double x = in_a ? A[own] : B[own];
        const int64_t a_lt = count_lt(A, n, x), a_le = count_le(A, n, x);
        const int64_t b_lt = count_lt(B, m, x), b_le = count_le(B, m, x);
        const int64_t dd = a_le * m - b_le * n;
        ks_plus = dd > ks_plus ? dd : ks_plus;
        ks_minus = -dd > ks_minus ? -dd : ks_minus;
        if (in_a) u2 += b_lt + b_le;
        // a tie group is counted by its first element: of A, or of B where A holds no equal value
        if (in_a ? a_lt == own : (b_lt == own && a_le == a_lt)) {
          const int64_t g = (a_le - a_lt) + (b_le - b_lt);
          tie += g * g * g - g;
        }
      }
      ks_plus = uniform64(wave_max64(ks_plus));
      ks_minus = uniform64(wave_max64(ks_minus));
      u2 = wave_sum((long long)u2);
      tie = wave_sum((long long)tie);
      const int64_t p = n < m ? n : m, P = n < m ? m : n;
      if (p <= MAX_SMALL && P <= exact_cells / p)  // n m <= exact_cells, without the product
        ks_p = ks_exact_p(lane, p, P, ks_plus > ks_minus ? ks_plus : ks_minus);
    }
    if (lane == 0) {
      out_n_a[t] = n;
      out_n_b[t] = m;
      out_ks_plus[t] = ks_plus;
      out_ks_minus[t] = ks_minus;
      out_u2[t] = u2;
      out_tie[t] = tie;
      out_ks_p[t] = ks_p;
    }
  }
}

}  // namespace

extern "C" int nvk_site_rank_tests_dev(nvk_ctx *ctx, int64_t n_rows_a, const int64_t *key_a, const double *val_a,
                                       int64_t n_rows_b, const int64_t *key_b, const double *val_b, int64_t n_sites,
                                       const int64_t *site_key, int64_t exact_cells, int64_t *out_n_a,
                                       int64_t *out_n_b, int64_t *out_ks_plus, int64_t *out_ks_minus, int64_t *out_u2,
                                       int64_t *out_tie, double *out_ks_p) {
  const char *what = "nvk_site_rank_tests_dev";
  int rc = check_site_samples(what, ctx, n_rows_a, key_a, val_a, n_rows_b, key_b, val_b, n_sites, site_key);
  if (rc) return rc;
  if (exact_cells < 0) {
    nvk_set_error("%s: invalid argument (exact_cells >= 0)", what);
    return NVK_ERR_INVALID;
  }
  if (n_sites == 0) return NVK_OK;
  if (!out_n_a || !out_n_b || !out_ks_plus || !out_ks_minus || !out_u2 || !out_tie || !out_ks_p) {
    nvk_set_error("%s: NULL output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  return nvk_timed(ctx, NVK_K_SITE, [&] {
    hipLaunchKernelGGL(site_rank_tests_kernel, dim3(grid_of(n_sites, NT / 64)), dim3(NT), 0, ctx->stream, n_rows_a,
                       key_a, val_a, n_rows_b, key_b, val_b, n_sites, site_key, exact_cells, out_n_a, out_n_b,
                       out_ks_plus, out_ks_minus, out_u2, out_tie, out_ks_p);
  });
}
