// The k-mer HMM as the Viterbi sweep (kernels_decode.hip) and the forward-backward sweeps (kernels_posterior.hip) lay
// it out, stated once: 4^k states, one workgroup per read, thread u owning the 16 consecutive states 16 u .. 16 u + 15
// with their table entries in registers, rows of the trellis in LDS padded by HMM_PAD doubles after every 16 entries
// (kernels_decode.hip says why); the shared part of the entries' arguments and checks; the Gaussian log density, and
// the emission floor and EXP of the linear-domain sweeps.
#pragma once
#include <type_traits>

#include "nvk_internal.h"
#include "xmath.h"

constexpr int HMM_MAX_EVENTS = 1 << 26;  // per read
constexpr int HMM_PAD = 2;               // doubles of padding after every 16 entries of a row in LDS

// S states, T threads, Q = S / 4, ROW doubles of a padded row; a workgroup is NW waves, W lanes of each hold a thread
template <int K>
struct KmerHmm {
  static constexpr int S = 1 << (2 * K), T = S / 16, Q = S / 4, ROW = S + T * HMM_PAD;
  static constexpr int W = T < 64 ? T : 64, NW = T / W;
};

// where entry s lies in a padded row
__device__ __forceinline__ constexpr int hmm_at(int s) { return s + (s >> 4) * HMM_PAD; }

// what every sweep reads; the leading part of DecodeArgs and PostArgs
struct HmmIn {
  const double *level;  // the events' levels, read r at ev_off[r]
  const int64_t *ev_off;
  const double *mean, *ac, *mc;  // the table, f64[4^k]
  const int32_t *status_in;      // per read or null
};

// status of read rd of E events, as every sweep sees it
__device__ __forceinline__ int hmm_status(const HmmIn &in, int64_t rd, int E) {
  const int status = in.status_in ? in.status_in[rd] : 0;
  return (status == 0 && E == 0) ? NVK_DEC_NO_EVENTS : status;
}

// thread u's 16 table entries; first(j) runs right after entry j is loaded (a second loop takes other registers)
template <class F>
__device__ __forceinline__ void hmm_load_table(const HmmIn &in, int u, double (&mean)[16], double (&ac)[16],
                                               double (&mc)[16], F &&first) {
#pragma unroll
  for (int j = 0; j < 16; j++) {
    mean[j] = in.mean[16 * u + j];
    ac[j] = in.ac[16 * u + j];
    mc[j] = in.mc[16 * u + j];
    first(j);
  }
}

// log of the Gaussian of (mean, ac, mc) at level e
__device__ __forceinline__ double gauss_log(double e, double mean, double ac, double mc) {
  const double d = e - mean;
  return ac - (d * d) * mc;
}

// The linear-domain sweeps (kernels_posterior.hip, kernels_repeatlik.hip): an emission below the floor counts as the
// floor, and EXP of the K-MER POSTERIORS contract (include/nadavca_hip.h)
constexpr double POST_EM_FLOOR = -300.0;
__device__ __forceinline__ double post_exp(double g) {
  const double y = g * xm::LOG2E;
  const double n = rint(y);
  return ldexp(xm::exp2_frac_horner(y - n), (int)n);
}

// f(std::integral_constant<int, K>{}) for the K that k is, 2..6 (checked by hmm_check_entry)
template <class F>
void hmm_dispatch_k(int k, F &&f) {
  switch (k) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 6>{}); break;
  }
}

// the checks the two entry points share; `pos_name`: what the entry calls the position inside the state
inline int hmm_check_entry(const char *what, nvk_ctx *ctx, int k, const char *pos_name, int pos, int64_t n_reads,
                           int64_t total_events, const double *level, const int64_t *ev_off, const double *mean,
                           const double *ac, const double *mc) {
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (k < 2 || k > 6) {
    nvk_set_error("%s: k %d is outside 2..6", what, k);
    return NVK_ERR_UNSUPPORTED;
  }
  if (pos < 0 || pos >= k) {
    nvk_set_error("%s: %s %d is outside 0..k-1 (k %d)", what, pos_name, pos, k);
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff || total_events < 0) {
    nvk_set_error("%s: n_reads %lld or total_events %lld out of range", what, (long long)n_reads,
                  (long long)total_events);
    return NVK_ERR_INVALID;
  }
  if (!ev_off || (total_events > 0 && !level) || !mean || !ac || !mc) {
    nvk_set_error("%s: NULL levels, offsets or table", what);
    return NVK_ERR_INVALID;
  }
  return NVK_OK;
}
