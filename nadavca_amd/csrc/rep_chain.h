// What the two operators on a repeat's chain share (kernels_repeats.hip: the Viterbi count; kernels_repeatlik.hip: the
// likelihood of every count): the states per lane, a wave-uniform lane's value, and the host's checks of chains and
// items, which include/nadavca_hip.h states once (REPEAT COUNT).
#pragma once
#include <vector>

#include "nvk_internal.h"

constexpr int REP_MIN_STATES = 3;
constexpr int REP_MAX_EVENTS = 1 << 26;  // per item

// the instantiation that serves a chain of N states: the states a lane owns
__host__ __device__ constexpr int rep_spl(int N) { return N <= 64 ? 1 : N <= 128 ? 2 : 4; }

// the value lane `l` holds, l wave-uniform
__device__ __forceinline__ double rep_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// st_off, chain_par and items copied to the host and checked as the contract says -> NVK_OK and used[spl]: whether
// some item's chain needs the instantiation of spl states per lane
inline int rep_check_batch(const char *what, nvk_ctx *ctx, int64_t n_items, const int64_t *items, int64_t total_events,
                           int64_t n_chains, int64_t total_states, const int64_t *st_off, const int32_t *chain_par,
                           bool (&used)[5]) {
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> soff;
  int rc = nvk_fetch_offsets(ctx, "state", st_off, n_chains, soff, "total_states", total_states);
  if (rc) return rc;
  std::vector<int32_t> par((size_t)n_chains * 4);
  std::vector<int64_t> item((size_t)n_items * 3);
  if (n_chains > 0)
    NVK_HIP(hipMemcpyAsync(par.data(), chain_par, par.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipMemcpyAsync(item.data(), items, item.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  for (int64_t c = 0; c < n_chains; c++) {
    const int64_t N = soff[c + 1] - soff[c];
    const int32_t lp_from = par[4 * c], lp_to = par[4 * c + 1], m1 = par[4 * c + 2], m2 = par[4 * c + 3];
    if (N > NVK_REP_MAX_STATES) {
      nvk_set_error("%s: chain %lld has %lld states, above %d", what, (long long)c, (long long)N,
                    (int)NVK_REP_MAX_STATES);
      return NVK_ERR_UNSUPPORTED;
    }
    if (N < REP_MIN_STATES || !(0 <= lp_to && lp_to < lp_from && lp_from < m2 && m2 <= N - 1 && 1 <= m1 && m1 <= m2)) {
      nvk_set_error("%s: chain %lld of %lld states has (lp_from, lp_to, m1, m2) = (%d, %d, %d, %d); wanted are at "
                    "least %d states, 0 <= lp_to < lp_from < m2 <= N - 1 and 1 <= m1 <= m2", what, (long long)c,
                    (long long)N, lp_from, lp_to, m1, m2, REP_MIN_STATES);
      return NVK_ERR_INVALID;
    }
  }
  for (bool &u : used) u = false;
  for (int64_t t = 0; t < n_items; t++) {
    const int64_t c = item[3 * t], lo = item[3 * t + 1], hi = item[3 * t + 2];
    if (c < 0 || c >= n_chains || lo < 0 || hi < lo || hi > total_events || hi - lo > REP_MAX_EVENTS) {
      nvk_set_error("%s: item %lld is (chain %lld, events %lld .. %lld); there are %lld chains and %lld events, and an "
                    "item takes at most %d", what, (long long)t, (long long)c, (long long)lo, (long long)hi,
                    (long long)n_chains, (long long)total_events, REP_MAX_EVENTS);
      return NVK_ERR_INVALID;
    }
    used[rep_spl((int)(soff[c + 1] - soff[c]))] = true;
  }
  return NVK_OK;
}
