// Per-site two-sample Gaussian mixture tests (nadavca_amd/site_mixtures.py): for every listed (position, strand) a
// two-component Gaussian mixture over the pooled values of one event column, the components shared by the two samples:
// first with one mixing weight (the fit never sees the labels; its responsibilities carry a permutation score test),
// then, from that solution, with one weight per sample (the stoichiometry).  The contract: include/nadavca_hip.h,
// nvk_site_mixture_tests_dev.
//
// Work split: ONE WAVE PER LISTED SITE (grid-stride), as kernels_siteranks.hip; the two runs of the site come from
// wave-uniform binary searches on the sorted keys.  Lanes stride over the pooled rows, A's run and then B's.  Every
// floating-point sum is a lane's loop over its rows in ascending order followed by a butterfly over the wave
// (wave_sum_dpp: wave_sum_n's additions, the sums of one sweep interleaved): the same bits on every run, whatever the
// launch.
//
// An EM step is two sweeps: the responsibilities and the sums for weight and means, then the squared deviations from
// the NEW means.  The centred values y = x - mean and, within a step, the responsibilities stay in registers while the
// site has at most 64 * CACHE rows; beyond that every sweep reads the values again and recomputes the responsibility
// from the step's parameters.  Both paths run the same expressions in the same order (the library is built with
// -ffp-contract=off) and give the same bits.  Per row and sweep there is one exp, of a number <= 0; the two logarithms
// and reciprocals of the standard deviations are wave-uniform.  Only the two likelihood sweeps, one per stage, take a
// logarithm per row.
//
// At sequencing coverage (10 .. 40 per strand and sample) a third to all of the wave's lanes hold a row, and the
// wave-uniform part of a step (logarithms, roots, divisions) is computed by every lane; DESIGN.md 4.7 has the time.
// Resources on gfx950: no LDS, no scratch, no atomics; the register counts are in DESIGN.md 4.7.
#include <math.h>

#include "site_runs.h"

namespace {

constexpr int NT = 256;
constexpr int CACHE = 2;  // rows per lane whose y and r stay in registers: sites of up to 64 * CACHE rows
constexpr int N_COUNTS = 5, N_FIT = 17;             // the columns of out_counts and out_fit
constexpr double HALF_LOG_2PI = 0.9189385332046727;  // log(2 pi) / 2

// The butterfly of wave_sum_n (every lane ends with p[l] + p[l xor d] for d = 32, 16, 8, 4, 2, 1, the same additions in
// the same order, so the same bits) with the four distances inside a 16-lane row on DPP moves instead of trips through
// the LDS crossbar: an EM step is a chain of two such butterflies, and their latency is most of what a step waits for.
template <int CTRL, int BANKS>
__device__ __forceinline__ double dpp_take(double old, double v) {
  int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xf, BANKS, false);
  int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xf, BANKS, false);
  return __hiloint2double(hi, lo);
}
template <int D>
__device__ __forceinline__ double lane_xor(double v) {
  if (D == 8) return dpp_take<0x128, 0xf>(v, v);  // row_ror:8
  if (D == 4)                                     // row_shl:4 into the lanes with bit 2 clear, row_shr:4 into the others
    return dpp_take<0x114, 0xa>(dpp_take<0x104, 0x5>(v, v), v);
  if (D == 2) return dpp_take<0x4e, 0xf>(v, v);   // quad_perm:[2,3,0,1]
  if (D == 1) return dpp_take<0xb1, 0xf>(v, v);   // quad_perm:[1,0,3,2]
  return __shfl_xor(v, D, 64);
}
template <int D, int N>
__device__ __forceinline__ void butterfly_step(double (&v)[N]) {
  double o[N];
#pragma unroll
  for (int a = 0; a < N; a++) o[a] = lane_xor<D>(v[a]);
#pragma unroll
  for (int a = 0; a < N; a++) v[a] += o[a];
}
template <int N>
__device__ __forceinline__ void wave_sum_dpp(double (&v)[N]) {
  butterfly_step<32>(v);
  butterfly_step<16>(v);
  butterfly_step<8>(v);
  butterfly_step<4>(v);
  butterfly_step<2>(v);
  butterfly_step<1>(v);
}

// the mixture: component means (centred) and standard deviations, the weight of component 1 per sample
struct Mix {
  double m0, sd0, m1, sd1, wa, wb;
};
// what an E-step derives from it once per wave
struct Derived {
  double i0, i1, ls0, ls1;
};
__device__ __forceinline__ Derived derive(const Mix &p) {
  return {1.0 / p.sd0, 1.0 / p.sd1, log(p.sd0), log(p.sd1)};
}

// The responsibility of component 1 for a row of centred value y and weight w, from e = exp(-|q|) only.  WITH_LL:
// *ll = the row's log density without the - log(2 pi) / 2.
template <bool WITH_LL>
__device__ __forceinline__ double responsibility(double y, double w, const Mix &p, const Derived &d, double *ll) {
  const double z0 = (y - p.m0) * d.i0, z1 = (y - p.m1) * d.i1;
  const double l0 = -0.5 * (z0 * z0) - d.ls0, l1 = -0.5 * (z1 * z1) - d.ls1;
  const double q = l1 - l0;
  const bool pos = q > 0.0;
  const double e = exp(-fabs(q));
  const double u = 1.0 - w;
  const double we = w * e;
  const double num = pos ? w : we;
  const double den = pos ? w + u * e : we + u;
  if (WITH_LL) *ll = (pos ? l1 : l0) + log(den);
  return den > 0.0 ? num / den : (pos ? 0.0 : 1.0);
}

// One site with rows on both sides: A (n values), B (m values).  Every lane calls it with the same arguments; lane 0
// writes counts[2 .. 5) and fit[0 .. 17).
template <bool CACHED>
__device__ __forceinline__ void fit_site(int lane, const double *A, int64_t n, const double *B, int64_t m,
                                         int iterations, double min_sd_ratio, int64_t *counts, double *fit) {
  const int64_t N = n + m;
  const double fN = (double)N;
  double yc[CACHED ? CACHE : 1], rc[CACHED ? CACHE : 1];
  double mu = 0.0;
  auto value = [&](int64_t i) { return i < n ? A[i] : B[i - n]; };
  // fn(y, in_a, r): a sweep over the lane's rows, ascending; r is the row's slot of the responsibility cache
  auto sweep = [&](auto &&fn) {
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < CACHE; j++)
        if (lane + 64 * j < N) fn(yc[j], lane + 64 * j < n, rc[j]);
    } else {
      for (int64_t i = lane; i < N; i += 64) fn(value(i) - mu, i < n, rc[0]);
    }
  };

  // one component
  {
    double s[1] = {0.0};
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < CACHE; j++) {
        yc[j] = lane + 64 * j < N ? value(lane + 64 * j) : 0.0;
        if (lane + 64 * j < N) s[0] += yc[j];
      }
    } else {
      for (int64_t i = lane; i < N; i += 64) s[0] += value(i);
    }
    wave_sum_dpp(s);
    mu = s[0] / fN;
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < CACHE; j++) yc[j] -= mu;
    }
  }
  double a[4] = {0.0, 0.0, 0.0, 0.0};  // sum y^2; the rows above the mean, their sum of y, the sum of y of the others
  sweep([&](double y, bool, double &) {
    const bool hi = y > 0.0;
    a[0] += y * y;
    a[1] += hi ? 1.0 : 0.0;
    a[2] += hi ? y : 0.0;
    a[3] += hi ? 0.0 : y;
  });
  wave_sum_dpp(a);
  const double s = sqrt(a[0] / fN);
  const double ll_one = -fN * (log(s) + (HALF_LOG_2PI + 0.5));
  const double c1 = a[1], c0 = fN - a[1];
  if (!(s > 0.0) || !(s < INFINITY) || !(c0 > 0.0) || !(c1 > 0.0)) {
    if (lane == 0) {
      counts[2] = counts[3] = counts[4] = 0;
#pragma unroll
      for (int f = 0; f < N_FIT; f++) fit[f] = NAN;
      fit[0] = fit[6] = fit[16] = ll_one;
    }
    return;
  }
  const double sd_min = min_sd_ratio * s;

  // start: the rows at or below the mean, and those above it
  Mix p;
  p.m0 = a[3] / c0;
  p.m1 = a[2] / c1;
  {
    double v[2] = {0.0, 0.0};
    sweep([&](double y, bool, double &) {
      const bool hi = y > 0.0;
      const double d = y - (hi ? p.m1 : p.m0);
      v[0] += hi ? 0.0 : d * d;
      v[1] += hi ? d * d : 0.0;
    });
    wave_sum_dpp(v);
    p.sd0 = fmax(sqrt(v[0] / c0), sd_min);
    p.sd1 = fmax(sqrt(v[1] / c1), sd_min);
  }
  p.wa = p.wb = c1 / fN;

  if (lane == 0) {
    counts[2] = 1;
    fit[0] = ll_one;
  }
  // stage 0: one weight for all rows (the labels are not looked at); stage 1: from its solution, one weight per sample
#pragma unroll 1
  for (int stage = 0; stage < 2; stage++) {
    const bool free = stage != 0;
    int steps = 0;
#pragma unroll 1
    for (int it = 0; it < iterations; it++) {
      const Derived d = derive(p);
      double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // sum r over A, over B, sum (1 - r), sum r y, sum (1 - r) y
      sweep([&](double y, bool in_a, double &keep) {
        const double r = responsibility<false>(y, in_a ? p.wa : p.wb, p, d, nullptr);
        if (CACHED) keep = r;
        const double r0 = 1.0 - r;
        t[0] += in_a ? r : 0.0;
        t[1] += in_a ? 0.0 : r;
        t[2] += r0;
        t[3] += r * y;
        t[4] += r0 * y;
      });
      wave_sum_dpp(t);
      const double r1 = t[0] + t[1], r0 = t[2];
      if (!(r1 > 0.0) || !(r0 > 0.0)) break;  // a component without rows: the stage ends with the step's parameters
      const double m0 = t[4] / r0, m1 = t[3] / r1;
      double v[2] = {0.0, 0.0};
      sweep([&](double y, bool in_a, double &keep) {
        const double r = CACHED ? keep : responsibility<false>(y, in_a ? p.wa : p.wb, p, d, nullptr);
        const double d0 = y - m0, d1 = y - m1;
        v[0] += (1.0 - r) * (d0 * d0);
        v[1] += r * (d1 * d1);
      });
      wave_sum_dpp(v);
      p.m0 = m0;
      p.m1 = m1;
      p.sd0 = fmax(sqrt(v[0] / r0), sd_min);
      p.sd1 = fmax(sqrt(v[1] / r1), sd_min);
      p.wa = free ? t[0] / (double)n : r1 / fN;
      p.wb = free ? t[1] / (double)m : r1 / fN;
      steps++;
    }
    // the stage's log-likelihood and the responsibilities' sums over A and over B at its solution
    const Derived d = derive(p);
    double t[3] = {0.0, 0.0, 0.0};
    sweep([&](double y, bool in_a, double &keep) {
      double ll;
      const double r = responsibility<true>(y, in_a ? p.wa : p.wb, p, d, &ll);
      if (CACHED) keep = r;
      t[0] += ll;
      t[1] += in_a ? r : 0.0;
      t[2] += in_a ? 0.0 : r;
    });
    wave_sum_dpp(t);
    const double ll = t[0] - fN * HALF_LOG_2PI;
    double *out = fit + (free ? 10 : 1);
    if (lane == 0) {
      counts[3 + stage] = steps;
      out[0] = mu + p.m0;
      out[1] = p.sd0;
      out[2] = mu + p.m1;
      out[3] = p.sd1;
      out[4] = p.wa;
      out[5] = free ? p.wb : ll;
      if (free) out[6] = ll;
    }
    if (!free) {
      // the score sums: the stage-0 responsibilities are fixed scores under exchangeable labels
      const double mean_r = (t[1] + t[2]) / fN;
      double v[1] = {0.0};
      sweep([&](double y, bool in_a, double &keep) {
        const double r = CACHED ? keep : responsibility<false>(y, in_a ? p.wa : p.wb, p, d, nullptr);
        const double dr = r - mean_r;
        v[0] += dr * dr;
      });
      wave_sum_dpp(v);
      if (lane == 0) {
        fit[7] = t[1];
        fit[8] = t[2];
        fit[9] = v[0];
      }
    }
  }
}

// one wave per listed site (grid-stride)
__global__ __launch_bounds__(NT) void site_mixture_tests_kernel(int64_t n_rows_a, const int64_t *key_a,
                                                                const double *val_a, int64_t n_rows_b,
                                                                const int64_t *key_b, const double *val_b,
                                                                int64_t n_sites, const int64_t *site_key,
                                                                int iterations, double min_sd_ratio,
                                                                int64_t *out_counts, double *out_fit) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wave; t < n_sites; t += waves) {
    const auto [la, n, lb, m] = site_runs(key_a, n_rows_a, key_b, n_rows_b, site_key[t]);
    int64_t *counts = out_counts + (size_t)t * N_COUNTS;
    double *fit = out_fit + (size_t)t * N_FIT;
    if (lane == 0) {
      counts[0] = n;
      counts[1] = m;
    }
    if (n == 0 || m == 0) {
      if (lane < 3) counts[2 + lane] = 0;
      if (lane < N_FIT) fit[lane] = NAN;
      continue;
    }
    if (n + m <= 64 * CACHE)
      fit_site<true>(lane, val_a + la, n, val_b + lb, m, iterations, min_sd_ratio, counts, fit);
    else
      fit_site<false>(lane, val_a + la, n, val_b + lb, m, iterations, min_sd_ratio, counts, fit);
  }
}

}  // namespace

extern "C" int nvk_site_mixture_tests_dev(nvk_ctx *ctx, int64_t n_rows_a, const int64_t *key_a, const double *val_a,
                                          int64_t n_rows_b, const int64_t *key_b, const double *val_b, int64_t n_sites,
                                          const int64_t *site_key, int iterations, double min_sd_ratio,
                                          int64_t *out_counts, double *out_fit) {
  const char *what = "nvk_site_mixture_tests_dev";
  int rc = check_site_samples(what, ctx, n_rows_a, key_a, val_a, n_rows_b, key_b, val_b, n_sites, site_key);
  if (rc) return rc;
  if (iterations < 1 || iterations > 1024 || !(min_sd_ratio > 0.0) || !(min_sd_ratio <= 1.0)) {
    nvk_set_error("%s: iterations %d, min_sd_ratio %g outside the served range (1 <= iterations <= 1024, 0 < "
                  "min_sd_ratio <= 1)", what, iterations, min_sd_ratio);
    return NVK_ERR_INVALID;
  }
  if (n_sites == 0) return NVK_OK;
  if (!out_counts || !out_fit) {
    nvk_set_error("%s: NULL output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  return nvk_timed(ctx, NVK_K_SITE, [&] {
    hipLaunchKernelGGL(site_mixture_tests_kernel, dim3(grid_of(n_sites, NT / 64)), dim3(NT), 0, ctx->stream, n_rows_a,
                       key_a, val_a, n_rows_b, key_b, val_b, n_sites, site_key, iterations, min_sd_ratio, out_counts,
                       out_fit);
  });
}
