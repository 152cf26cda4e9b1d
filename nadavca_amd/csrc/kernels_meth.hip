// detect_meth's scoring of pattern occurrences (nadavca/detect_meth.py:21-65: calculate_meth_scores + maxs3) for
// every read of a batch, on the device:
//
//   nvk_meth_count_dev    per read, the number of scorable occurrences of the pattern
//   nvk_meth_scores_dev   their positions, the 11 event scores of each and the aggregate, at offsets the caller
//                         takes from the counts with a prefix sum
//
// One wave64 per read; its lanes walk the read's reference part 64 positions at a time.  An occurrence is found
// and checked by each lane on its own; __ballot gives the wave the occurrence mask and a popcount of its lower bits
// gives each lane its slot, so the occurrences of a read are written in ascending position without atomics and the
// output is the same on every run.  Both passes run the same search (one template), so the counts and the slots
// agree by construction.  About 20 bytes per reference position: a small latency-bound pass, not tuned.
//
// Arithmetic as the host's: z = |mean - expected| / 0.35287208, score = -log(max(1e-50, erfc(z / sqrt 2))), which
// is 2 * ndtr(-z) (scipy's ndtr takes this same erfc for z >= 1, and 0.5 + 0.5 * erf below); the aggregate is the
// largest of the nine sums (s[i] + s[i+1]) + s[i+2] in Python's order (-ffp-contract=off keeps it so).
#include <math.h>

#include <vector>

#include "nvk_internal.h"

namespace {

constexpr int NT = 256;
constexpr int FLANK = 5;                // events on each side of the occurrence's first base (detect_meth.py:42)
constexpr int WIN = 2 * FLANK + 1;      // events scored per occurrence
constexpr double LEVEL_SD = 0.35287208;  // detect_meth.py:24
constexpr double SMALLEST_PVAL = 1e-50;  // detect_meth.py:21

// EMIT = false: out_count[rd] = number of scorable occurrences of read rd.  EMIT = true: occurrence k of read rd
// (ascending position) goes to slot occ_off[rd] + k, as long as k < occ_off[rd+1] - occ_off[rd].
template <bool EMIT>
__global__ __launch_bounds__(NT) void meth_kernel(int64_t n_reads, const int32_t *reference, const int64_t *ref_off,
                                                  const double *means, const double *expected,
                                                  const int32_t *status, const int32_t *pattern, int64_t m,
                                                  int64_t *out_count, const int64_t *occ_off, int64_t *out_pos,
                                                  double *out_scores, double *out_aggregate) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t rd = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); rd < n_reads; rd += waves) {
    const int64_t r0 = ref_off[rd], R = ref_off[rd + 1] - r0;
    const bool live = !status || status[rd] == 0;
    int64_t base = 0, cap = 0;
    if (EMIT) {
      base = occ_off[rd];
      cap = occ_off[rd + 1] - base;
    }
    int64_t n = 0;  // occurrences of this read before the current 64 positions (wave-uniform)
    for (int64_t p0 = 0; live && p0 < R; p0 += 64) {
      const int64_t p = p0 + lane;
      // str.find semantics: the pattern at p (overlaps allowed, the empty pattern everywhere); scorable when
      // the 11 events p-5 .. p+5 exist and none is empty (NaN mean)
      bool occ = p >= FLANK && p + FLANK < R && p + m <= R;
      for (int64_t q = 0; occ && q < m; q++) {
        const int32_t c = pattern[q];
        occ = c >= 0 && c <= 3 && c == reference[r0 + p + q];
      }
      for (int i = -FLANK; occ && i <= FLANK; i++) occ = !isnan(means[r0 + p + i]);
      const unsigned long long mask = __ballot(occ);
      if (EMIT && occ) {
        const int64_t slot = n + __popcll(mask & ((1ull << lane) - 1ull));
        if (slot < cap) {
          const int64_t o = base + slot;
          double s[WIN];
          for (int i = 0; i < WIN; i++) {
            const int64_t g = r0 + p - FLANK + i;
            const double z = fabs(means[g] - expected[g]) / LEVEL_SD;
            const double pv = erfc(z * M_SQRT1_2);
            s[i] = -log(pv < SMALLEST_PVAL ? SMALLEST_PVAL : pv);
            out_scores[WIN * o + i] = s[i];
          }
          double agg = (s[0] + s[1]) + s[2];
          for (int i = 1; i + 2 < WIN; i++) {
            const double v = (s[i] + s[i + 1]) + s[i + 2];
            agg = v > agg ? v : agg;
          }
          out_pos[o] = p;
          out_aggregate[o] = agg;
        }
      }
      n += __popcll(mask);
    }
    if (!EMIT && lane == 0) out_count[rd] = n;
  }
}

// The checks both entry points share.  ref_off is a device array: it is copied to the host to be checked
// (8 bytes per read), and it must end at total_ref.
int meth_check(const char *what, nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int32_t *reference,
               const int64_t *ref_off, const double *means, const int32_t *pattern, int64_t pattern_len) {
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff || total_ref < 0) {
    nvk_set_error("%s: n_reads %lld or total_ref %lld out of range", what, (long long)n_reads,
                  (long long)total_ref);
    return NVK_ERR_INVALID;
  }
  if (pattern_len < 0 || (pattern_len > 0 && !pattern)) {
    nvk_set_error("%s: pattern_len %lld is negative or the pattern is NULL", what, (long long)pattern_len);
    return NVK_ERR_INVALID;
  }
  if (!ref_off || (total_ref > 0 && (!reference || !means))) {
    nvk_set_error("%s: NULL reference, offsets or means", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  return nvk_fetch_offsets(ctx, "reference", ref_off, n_reads, off, "total_ref", total_ref);
}

}  // namespace

extern "C" int nvk_meth_count_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int32_t *reference,
                                  const int64_t *ref_off, const double *means, const int32_t *status,
                                  const int32_t *pattern, int64_t pattern_len, int64_t *out_count) {
  int rc = meth_check("nvk_meth_count_dev", ctx, n_reads, total_ref, reference, ref_off, means, pattern,
                      pattern_len);
  if (rc) return rc;
  if (n_reads == 0) return NVK_OK;
  if (!out_count) {
    nvk_set_error("nvk_meth_count_dev: out_count is NULL");
    return NVK_ERR_INVALID;
  }
  return nvk_timed(ctx, NVK_K_METH, [&] {
    hipLaunchKernelGGL(meth_kernel<false>, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads,
                       reference, ref_off, means, (const double *)nullptr, status, pattern, pattern_len, out_count,
                       (const int64_t *)nullptr, (int64_t *)nullptr, (double *)nullptr, (double *)nullptr);
  });
}

extern "C" int nvk_meth_scores_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int32_t *reference,
                                   const int64_t *ref_off, const double *means, const double *expected,
                                   const int32_t *status, const int32_t *pattern, int64_t pattern_len,
                                   const int64_t *occ_off, int64_t *out_pos, double *out_scores,
                                   double *out_aggregate) {
  int rc = meth_check("nvk_meth_scores_dev", ctx, n_reads, total_ref, reference, ref_off, means, pattern,
                      pattern_len);
  if (rc) return rc;
  if (total_ref > 0 && !expected) {
    nvk_set_error("nvk_meth_scores_dev: expected is NULL");
    return NVK_ERR_INVALID;
  }
  std::vector<int64_t> off;
  if ((rc = nvk_fetch_offsets(ctx, "occurrence", occ_off, n_reads, off))) return rc;
  if (off[n_reads] == 0) return NVK_OK;
  if (!out_pos || !out_scores || !out_aggregate) {
    nvk_set_error("nvk_meth_scores_dev: NULL output");
    return NVK_ERR_INVALID;
  }
  return nvk_timed(ctx, NVK_K_METH, [&] {
    hipLaunchKernelGGL(meth_kernel<true>, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads,
                       reference, ref_off, means, expected, status, pattern, pattern_len, (int64_t *)nullptr,
                       occ_off, out_pos, out_scores, out_aggregate);
  });
}
