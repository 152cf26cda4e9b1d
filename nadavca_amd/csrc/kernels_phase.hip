// Phasing of heterozygous sites and haplotype tags of reads (nadavca_amd/phase.py): the three floating-point steps of
// the loop whose contract is in include/nadavca_hip.h (nvk_phase_links_dev).  The integer work between them (blocks,
// starting phase, flips) is torch on the device.
//
//   nvk_phase_links_dev   per site s >= 1: the log-likelihood ratio "the alternatives of s - 1 and s lie on one
//                         haplotype" against "on different ones" over the reads that have evidence at both, and their
//                         number
//   nvk_phase_tag_dev     per read: its block, the signed evidence H for haplotype 1 of that block, its sites there
//   nvk_phase_votes_dev   per site: the leave-one-out vote of the reads tagged in its block
//
// The evidence of a read at a site is the clipped value d of nvk_allele_rows_dev for (read, position, alternative
// base).  The site kernels read it from the rows in stable key order (a site's rows are contiguous, its reads ascend),
// the read kernel from the read-major rows (a read's row of a position is found by arithmetic).
//
// No floating-point atomics, as in kernels_allele.hip: a site's sum is a lane's loop over rows l, l + 64, ... in
// ascending order followed by wave_sum's butterfly; a read's H is one thread's left-to-right sum.  Two runs give the
// same bits.
//
// Work split: ONE WAVE PER SITE (grid-stride) in the site kernels; a site has tens of rows, so about half a wave
// idles, the price of sums whose order does not depend on the launch.  The links kernel finds a row's read among the
// previous site's rows by binary search over their read indices (log2(coverage) dependent loads per row).  ONE THREAD
// PER READ in the tag kernel: a read meets a handful of sites, found by two binary searches over the site positions.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.8.
#include <math.h>

#include <vector>

#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int NT = 256;

// min(max(d, -clip), clip); -inf and a d that is not a number give -clip
__device__ __forceinline__ double clipped(double d, double clip) { return d > -clip ? (d < clip ? d : clip) : -clip; }

// log(exp(a) + exp(b))
__device__ __forceinline__ double lae(double a, double b) { return fmax(a, b) + log1p(exp(-fabs(a - b))); }

// one wave per site (grid-stride)
__global__ __launch_bounds__(NT) void phase_links_kernel(int64_t n_sites, int alpha, const int64_t *site_lo,
                                                         const int64_t *site_hi, const int32_t *site_alt,
                                                         const int32_t *chain, const int64_t *row_read,
                                                         const double *val, double clip, double *out_link,
                                                         int64_t *out_shared) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t s = (int64_t)blockIdx.x * (NT / 64) + wave; s < n_sites; s += waves) {
    double acc = 0.0;
    int count = 0;
    if (s > 0 && chain[s] != 0) {
      const int64_t lo = site_lo[s], n = site_hi[s] - lo;
      const int64_t plo = site_lo[s - 1], pn = site_hi[s - 1] - plo;
      const int a1 = site_alt[s - 1], a2 = site_alt[s];
      if (a1 >= 0 && a1 < alpha && a2 >= 0 && a2 < alpha && pn > 0) {
        for (int64_t j = lane; j < n; j += 64) {
          const int64_t rd = row_read[lo + j];
          const int64_t q = lower_bound(row_read, plo, pn, rd);
          double term = 0.0;
          if (q < plo + pn && row_read[q] == rd) {
            const double e1 = clipped(val[(size_t)q * alpha + a1], clip);
            const double e2 = clipped(val[(size_t)(lo + j) * alpha + a2], clip);
            term = lae(e1 + e2, 0.0) - lae(e1, e2);
            count++;
          }
          acc += term;
        }
      }
      acc = wave_sum(acc);
      count = wave_sum(count);
    }
    if (lane == 0) {
      out_link[s] = acc;
      out_shared[s] = count;
    }
  }
}

// one thread per read (grid-stride)
__global__ __launch_bounds__(NT) void phase_tag_kernel(int64_t n_reads, int64_t n_sites, int alpha,
                                                       const int64_t *ref_off, const int64_t *chunk_start,
                                                       const int32_t *reverse, const int64_t *key, const double *val,
                                                       const int64_t *site_pos, const int32_t *site_alt,
                                                       const int64_t *site_block, const int32_t *site_sigma,
                                                       double clip, int64_t *out_block, double *out_llr,
                                                       int64_t *out_sites) {
  const int64_t threads = (int64_t)gridDim.x * NT;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_reads; i += threads) {
    const int64_t r0 = ref_off[i];
    const int64_t R = ref_off[i + 1] - r0;
    int64_t best_block = -1, best_n = 0;
    double best_h = 0.0;
    if (R > 0) {
      const int64_t c0 = chunk_start[i];
      const bool rev = reverse[i] != 0;
      const int64_t s0 = lower_bound(site_pos, 0, n_sites, c0);
      const int64_t s1 = lower_bound(site_pos, s0, n_sites - s0, c0 + R);
      int64_t block = -1, n = 0;
      double h = 0.0;
      // the run of the read's sites inside one block: kept when its |H| exceeds the best so far (the first on ties)
      auto close = [&]() {
        if (n > 0 && (best_n == 0 || fabs(h) > fabs(best_h))) {
          best_block = block;
          best_h = h;
          best_n = n;
        }
      };
      for (int64_t s = s0; s < s1; s++) {
        const int64_t P = site_pos[s];
        const int a = site_alt[s];
        if (P < c0 || P >= c0 + R || a < 0 || a >= alpha) continue;
        // forward columns need no flip; the rows of a reverse read run backwards (as consensus_kernel)
        const int64_t row = r0 + (rev ? R - 1 - (P - c0) : P - c0);
        if (key[row] != P) continue;
        const double e = clipped(val[(size_t)row * alpha + a], clip);
        const int64_t b = site_block[s];
        if (n == 0 || b != block) {
          close();
          block = b;
          h = 0.0;
          n = 0;
        }
        h += (double)site_sigma[s] * e;
        n++;
      }
      close();
    }
    out_block[i] = best_block;
    out_llr[i] = best_h;
    out_sites[i] = best_n;
  }
}

// one wave per site (grid-stride)
__global__ __launch_bounds__(NT) void phase_votes_kernel(int64_t n_sites, int alpha, const int64_t *site_lo,
                                                         const int64_t *site_hi, const int32_t *site_alt,
                                                         const int64_t *site_block, const int32_t *site_sigma,
                                                         const int64_t *row_read, const double *val,
                                                         const int64_t *read_block, const double *read_llr,
                                                         double clip, double *out_vote, int64_t *out_agree,
                                                         int64_t *out_against) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t s = (int64_t)blockIdx.x * (NT / 64) + wave; s < n_sites; s += waves) {
    const int64_t lo = site_lo[s], n = site_hi[s] - lo;
    const int a = site_alt[s];
    const int64_t block = site_block[s];
    const double sigma = (double)site_sigma[s];
    double acc = 0.0;
    int agree = 0, against = 0;
    if (a >= 0 && a < alpha) {
      for (int64_t j = lane; j < n; j += 64) {
        const int64_t rd = row_read[lo + j];
        double term = 0.0;
        if (read_block[rd] == block) {
          const double e = clipped(val[(size_t)(lo + j) * alpha + a], clip);
          // leave-one-out: the read's tag without this site's own share
          const double h = read_llr[rd] - sigma * e;
          if (h != 0.0) {
            term = h > 0.0 ? e : -e;
            const double side = term * sigma;
            agree += side > 0.0;
            against += side < 0.0;
          }
        }
        acc += term;
      }
    }
    acc = wave_sum(acc);
    agree = wave_sum(agree);
    against = wave_sum(against);
    if (lane == 0) {
      out_vote[s] = acc;
      out_agree[s] = agree;
      out_against[s] = against;
    }
  }
}

// the arguments the three entries share
int check_phase(const char *what, nvk_ctx *ctx, int64_t n_sites, int alphabet, double clip) {
  if (!ctx || n_sites < 0) {
    nvk_set_error("%s: invalid argument (ctx, n_sites >= 0)", what);
    return NVK_ERR_INVALID;
  }
  if (alphabet < 2 || alphabet > 8 || !(clip > 0.0) || !(clip < INFINITY)) {
    nvk_set_error("%s: alphabet %d, clip %g outside the served range (2 <= alphabet <= 8, 0 < clip < inf)", what,
                  alphabet, clip);
    return NVK_ERR_INVALID;
  }
  return NVK_OK;
}

}  // namespace

extern "C" int nvk_phase_links_dev(nvk_ctx *ctx, int64_t n_sites, int alphabet, const int64_t *site_lo,
                                   const int64_t *site_hi, const int32_t *site_alt, const int32_t *chain,
                                   const int64_t *row_read, const double *val, double clip, double *out_link,
                                   int64_t *out_shared) {
  const char *what = "nvk_phase_links_dev";
  int rc;
  if ((rc = check_phase(what, ctx, n_sites, alphabet, clip))) return rc;
  if (n_sites == 0) return NVK_OK;
  if (!site_lo || !site_hi || !site_alt || !chain || !row_read || !val || !out_link || !out_shared) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    hipLaunchKernelGGL(phase_links_kernel, dim3(grid_of(n_sites, NT / 64)), dim3(NT), 0, ctx->stream, n_sites,
                       alphabet, site_lo, site_hi, site_alt, chain, row_read, val, clip, out_link, out_shared);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_phase_tag_dev(nvk_ctx *ctx, int64_t n_reads, int64_t n_sites, int alphabet, const int64_t *ref_off,
                                 const int64_t *chunk_start, const int32_t *reverse, const int64_t *key,
                                 const double *val, const int64_t *site_pos, const int32_t *site_alt,
                                 const int64_t *site_block, const int32_t *site_sigma, double clip,
                                 int64_t *out_block, double *out_llr, int64_t *out_sites) {
  const char *what = "nvk_phase_tag_dev";
  int rc;
  if ((rc = check_phase(what, ctx, n_sites, alphabet, clip))) return rc;
  if (n_reads < 0 || n_reads > 0x7fffffff) {
    nvk_set_error("%s: n_reads %lld outside 0 .. 2^31 - 1", what, (long long)n_reads);
    return NVK_ERR_INVALID;
  }
  if (n_sites == 0 || n_reads == 0) return NVK_OK;
  if (!ref_off) {
    nvk_set_error("%s: offsets are NULL", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  if ((rc = nvk_fetch_offsets(ctx, "reference", ref_off, n_reads, off))) return rc;
  if (!chunk_start || !reverse || !site_pos || !site_alt || !site_block || !site_sigma || !out_block || !out_llr ||
      !out_sites || (off[n_reads] > 0 && (!key || !val))) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    hipLaunchKernelGGL(phase_tag_kernel, dim3(grid_of(n_reads, NT)), dim3(NT), 0, ctx->stream, n_reads, n_sites,
                       alphabet, ref_off, chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma,
                       clip, out_block, out_llr, out_sites);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_phase_votes_dev(nvk_ctx *ctx, int64_t n_sites, int alphabet, const int64_t *site_lo,
                                   const int64_t *site_hi, const int32_t *site_alt, const int64_t *site_block,
                                   const int32_t *site_sigma, const int64_t *row_read, const double *val,
                                   const int64_t *read_block, const double *read_llr, double clip, double *out_vote,
                                   int64_t *out_agree, int64_t *out_against) {
  const char *what = "nvk_phase_votes_dev";
  int rc;
  if ((rc = check_phase(what, ctx, n_sites, alphabet, clip))) return rc;
  if (n_sites == 0) return NVK_OK;
  if (!site_lo || !site_hi || !site_alt || !site_block || !site_sigma || !row_read || !val || !read_block ||
      !read_llr || !out_vote || !out_agree || !out_against) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    hipLaunchKernelGGL(phase_votes_kernel, dim3(grid_of(n_sites, NT / 64)), dim3(NT), 0, ctx->stream, n_sites,
                       alphabet, site_lo, site_hi, site_alt, site_block, site_sigma, row_read, val, read_block,
                       read_llr, clip, out_vote, out_agree, out_against);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
