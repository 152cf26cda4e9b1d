// The two runs of a listed site in the two samples' sorted keys, for the kernels that give one wave to a site
// (kernels_siteranks.hip, kernels_sitemix.hip).
#pragma once
#include "nvk_internal.h"
#include "wave.h"

// sample A's rows of the key are la .. la + n of its n_rows_a, sample B's lb .. lb + m; n and m wave-uniform
struct SiteRuns {
  int64_t la, n, lb, m;
};
__device__ __forceinline__ SiteRuns site_runs(const int64_t *key_a, int64_t n_rows_a, const int64_t *key_b,
                                              int64_t n_rows_b, int64_t q) {
  const int64_t la = lower_bound(key_a, 0, n_rows_a, q);
  const int64_t n = uniform64(lower_bound(key_a, la, n_rows_a - la, q + 1) - la);
  const int64_t lb = lower_bound(key_b, 0, n_rows_b, q);
  const int64_t m = uniform64(lower_bound(key_b, lb, n_rows_b - lb, q + 1) - lb);
  return {la, n, lb, m};
}
