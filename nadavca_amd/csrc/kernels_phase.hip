// Phasing of heterozygous sites and haplotype tags of reads (nadavca_amd/phase.py): the floating-point steps of the
// loop whose contracts are in include/nadavca_hip.h (nvk_phase_links_dev, nvk_phase_span_links_dev).  The integer work
// between them (blocks or the forest, starting phase, flips) is torch on the device.
//
//   nvk_phase_links_dev        per site s >= 1: the log-likelihood ratio "the alternatives of s - 1 and s lie on one
//                              haplotype" against "on different ones" over the reads that have evidence at both, and
//                              their number
//   nvk_phase_span_links_dev   per site s and w = 1 .. span: that link and those shared reads between sites s - w and s
//   nvk_phase_tag_dev          per read: its block, the signed evidence H for haplotype 1 of that block, its sites
//                              there; blocks are intervals of sites
//   nvk_phase_tag_blocks_dev   the same for any block array: the block with the largest |H| over ALL of the read's
//                              sites in that block (a singleton may sit inside another block)
//   nvk_phase_votes_dev        per site: the leave-one-out vote of the reads tagged in its block, for any block array
//
// The evidence of a read at a site is the clipped value d of nvk_allele_rows_dev for (read, position, alternative
// base).  The site kernels read it from the rows in stable key order (a site's rows are contiguous, its reads ascend),
// the read kernels from the read-major rows (a read's row of a position is found by arithmetic: ReadSites).
//
// No floating-point atomics, as in kernels_allele.hip: a site's sum is a lane's loop over rows l, l + 64, ... in
// ascending order followed by wave_sum's butterfly (wave_sum_n: the same additions per column); a read's H is one
// thread's left-to-right sum.  Two runs give the same bits, and every column of the links is the same sum whatever the
// span it is computed under.
//
// Work split: ONE WAVE PER SITE (grid-stride) in the site kernels; a site has tens of rows, so about half a wave
// idles, the price of sums whose order does not depend on the launch.  In the links kernel a lane loads its row's read
// index and its evidence at s ONCE and then finds the read among the rows of the W earlier sites by W binary searches
// over their read indices that advance in lockstep: the W loads of a step are independent and in flight together, so a
// step costs one memory round trip for all columns (log2(coverage) steps per row).  The columns live in registers,
// indexed statically (a template on 1 / 2 / 4 / 8 columns, the surplus masked by an empty range).  ONE THREAD PER READ
// in the tag kernels: a read meets a handful of sites, found by two binary searches over the site positions.
// phase_tag_kernel makes one pass and closes runs of equal blocks; phase_tag_blocks_kernel makes one pass per distinct
// block (ascending block index, found by the pass before), site_block staying in cache.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.8.
#include <math.h>

#include <vector>

#include "mix_mle.h"
#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int NT = 256;

// log(exp(a) + exp(b))
__device__ __forceinline__ double lae(double a, double b) { return fmax(a, b) + log1p(exp(-fabs(a - b))); }

// one wave per site (grid-stride); W >= span columns, column w - 1 for the site s - w.  The columns of s reach back to
// its first site: site_first[s], or with site_first null (span 1) s - 1 where chain[s] is set and s itself otherwise.
template <int W>
__global__ __launch_bounds__(NT) void phase_span_links_kernel(int64_t n_sites, int span, int alpha,
                                                              const int64_t *site_lo, const int64_t *site_hi,
                                                              const int32_t *site_alt, const int32_t *chain,
                                                              const int64_t *site_first, const int64_t *row_read,
                                                              const double *val, double clip, double *out_link,
                                                              int64_t *out_shared) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t s = (int64_t)blockIdx.x * (NT / 64) + wave; s < n_sites; s += waves) {
    double acc[W];
    int count[W];
    // the rows of the earlier sites (wave-uniform); an empty range where the column is not served
    int64_t plo[W], pn[W];
    int a1[W];
    const int64_t first = site_first ? site_first[s] : (chain[s] != 0 ? s - 1 : s);
    bool any = false;
#pragma unroll
    for (int w = 0; w < W; w++) {
      acc[w] = 0.0;
      count[w] = 0;
      plo[w] = 0;
      pn[w] = 0;
      a1[w] = 0;
      const int64_t p = s - (w + 1);
      // (p >= 0: site 0 with its chain flag set has no site before it)
      if (w < span && p >= 0 && p >= first) {
        const int a = site_alt[p];
        if (a >= 0 && a < alpha) {
          plo[w] = site_lo[p];
          pn[w] = site_hi[p] - plo[w];
          a1[w] = a;
          any = any || pn[w] > 0;
        }
      }
    }
    const int a2 = site_alt[s];
    if (any && a2 >= 0 && a2 < alpha) {
      const int64_t lo = site_lo[s], n = site_hi[s] - lo;
      for (int64_t j = lane; j < n; j += 64) {
        const int64_t rd = row_read[lo + j];
        const double e2 = clipped(val[(size_t)(lo + j) * alpha + a2], clip);
        // W lower bounds in lockstep: [L, H) stays inside [plo, plo + pn]
        int64_t L[W], H[W];
        bool open = false;
#pragma unroll
        for (int w = 0; w < W; w++) {
          L[w] = plo[w];
          H[w] = plo[w] + pn[w];
          open = open || L[w] < H[w];
        }
        while (open) {
          int64_t mid[W], got[W];
#pragma unroll
          for (int w = 0; w < W; w++) {
            mid[w] = (L[w] + H[w]) >> 1;
            got[w] = L[w] < H[w] ? row_read[mid[w]] : 0;
          }
          open = false;
#pragma unroll
          for (int w = 0; w < W; w++) {
            if (L[w] < H[w]) {
              if (got[w] < rd)
                L[w] = mid[w] + 1;
              else
                H[w] = mid[w];
            }
            open = open || L[w] < H[w];
          }
        }
        int64_t hit[W];
#pragma unroll
        for (int w = 0; w < W; w++) hit[w] = L[w] < plo[w] + pn[w] ? row_read[L[w]] : -1;
#pragma unroll
        for (int w = 0; w < W; w++) {
          double term = 0.0;
          if (L[w] < plo[w] + pn[w] && hit[w] == rd) {
            const double e1 = clipped(val[(size_t)L[w] * alpha + a1[w]], clip);
            term = lae(e1 + e2, 0.0) - lae(e1, e2);
            count[w]++;
          }
          acc[w] += term;
        }
      }
      wave_sum_n<W>(acc);
#pragma unroll
      for (int w = 0; w < W; w++) count[w] = wave_sum(count[w]);
    }
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < W; w++) {
        if (w < span) {
          out_link[s * span + w] = acc[w];
          out_shared[s * span + w] = count[w];
        }
      }
    }
  }
}

// What a read with rows meets: its rows r0 .. r0 + R (R > 0) of the read-major arrays, the position c0 of its first
// base, its strand, and the sites s0 .. s1 whose positions lie in [c0, c0 + R).
struct ReadSites {
  int64_t r0, R, c0, s0, s1;
  bool rev;
  __device__ ReadSites(int64_t r0_, int64_t R_, int64_t c0_, bool rev_, const int64_t *site_pos, int64_t n_sites)
      : r0(r0_), R(R_), c0(c0_), rev(rev_) {
    s0 = lower_bound(site_pos, 0, n_sites, c0);
    s1 = lower_bound(site_pos, s0, n_sites - s0, c0 + R);
  }
  // the read's row of site s where it has evidence there, -1 otherwise
  __device__ int64_t row_of(int64_t s, int alpha, const int64_t *site_pos, const int32_t *site_alt,
                            const int64_t *key) const {
    const int64_t P = site_pos[s];
    const int a = site_alt[s];
    if (P < c0 || P >= c0 + R || a < 0 || a >= alpha) return -1;
    // forward columns need no flip; the rows of a reverse read run backwards (as consensus_kernel)
    const int64_t row = r0 + (rev ? R - 1 - (P - c0) : P - c0);
    return key[row] == P ? row : -1;
  }
};

// one thread per read (grid-stride); blocks are intervals of sites
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
      const ReadSites rs(r0, R, chunk_start[i], reverse[i] != 0, site_pos, n_sites);
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
      for (int64_t s = rs.s0; s < rs.s1; s++) {
        const int64_t row = rs.row_of(s, alpha, site_pos, site_alt, key);
        if (row < 0) continue;
        const double e = clipped(val[(size_t)row * alpha + site_alt[s]], clip);
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

// one thread per read (grid-stride); any block array
__global__ __launch_bounds__(NT) void phase_tag_blocks_kernel(int64_t n_reads, int64_t n_sites, int alpha,
                                                              const int64_t *ref_off, const int64_t *chunk_start,
                                                              const int32_t *reverse, const int64_t *key,
                                                              const double *val, const int64_t *site_pos,
                                                              const int32_t *site_alt, const int64_t *site_block,
                                                              const int32_t *site_sigma, double clip,
                                                              int64_t *out_block, double *out_llr, int64_t *out_sites) {
  const int64_t threads = (int64_t)gridDim.x * NT;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_reads; i += threads) {
    const int64_t r0 = ref_off[i];
    const int64_t R = ref_off[i + 1] - r0;
    int64_t best_block = -1, best_n = 0;
    double best_h = 0.0;
    if (R > 0) {
      const ReadSites rs(r0, R, chunk_start[i], reverse[i] != 0, site_pos, n_sites);
      // the blocks of the read in ascending index: every pass sums the block `cur` and finds the next one
      bool more = false;
      int64_t cur = 0;
      for (int64_t s = rs.s0; s < rs.s1; s++) {
        if (rs.row_of(s, alpha, site_pos, site_alt, key) < 0) continue;
        const int64_t b = site_block[s];
        if (!more || b < cur) cur = b;
        more = true;
      }
      while (more) {
        bool has_next = false;
        int64_t next = 0, n = 0;
        double h = 0.0;
        for (int64_t s = rs.s0; s < rs.s1; s++) {
          const int64_t row = rs.row_of(s, alpha, site_pos, site_alt, key);
          if (row < 0) continue;
          const int64_t b = site_block[s];
          if (b == cur) {
            h += (double)site_sigma[s] * clipped(val[(size_t)row * alpha + site_alt[s]], clip);
            n++;
          } else if (b > cur && (!has_next || b < next)) {
            next = b;
            has_next = true;
          }
        }
        // the largest |H|, the smallest block index on ties (the blocks come in ascending index)
        if (best_n == 0 || fabs(h) > fabs(best_h)) {
          best_block = cur;
          best_h = h;
          best_n = n;
        }
        cur = next;
        more = has_next;
      }
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

// the arguments the five entries share
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

// the two links entries: the sites' first sites come as `chain` (span 1) or as `site_first`, the other one null
int phase_links(const char *what, nvk_ctx *ctx, int64_t n_sites, int span, int alphabet, const int64_t *site_lo,
                const int64_t *site_hi, const int32_t *site_alt, const int32_t *chain, const int64_t *site_first,
                const int64_t *row_read, const double *val, double clip, double *out_link, int64_t *out_shared) {
  int rc;
  if ((rc = check_phase(what, ctx, n_sites, alphabet, clip))) return rc;
  if (span < 1 || span > 8) {
    nvk_set_error("%s: span %d outside 1 .. 8", what, span);
    return NVK_ERR_INVALID;
  }
  if (n_sites == 0) return NVK_OK;
  if (!site_lo || !site_hi || !site_alt || (!chain && !site_first) || !row_read || !val || !out_link || !out_shared) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  return nvk_timed(ctx, NVK_K_ALLELE, [&] {
    const dim3 grid(grid_of(n_sites, NT / 64)), block(NT);
#define NVK_SPAN_LINKS(W)                                                                                       \
  hipLaunchKernelGGL(phase_span_links_kernel<W>, grid, block, 0, ctx->stream, n_sites, span, alphabet, site_lo, \
                     site_hi, site_alt, chain, site_first, row_read, val, clip, out_link, out_shared)
    if (span == 1)
      NVK_SPAN_LINKS(1);
    else if (span == 2)
      NVK_SPAN_LINKS(2);
    else if (span <= 4)
      NVK_SPAN_LINKS(4);
    else
      NVK_SPAN_LINKS(8);
#undef NVK_SPAN_LINKS
  });
}

// the two tag entries: the same arguments and checks, `kernel` one of the two tag kernels
int phase_tag(const char *what, decltype(&phase_tag_kernel) kernel, nvk_ctx *ctx, int64_t n_reads, int64_t n_sites,
              int alphabet, const int64_t *ref_off, const int64_t *chunk_start, const int32_t *reverse,
              const int64_t *key, const double *val, const int64_t *site_pos, const int32_t *site_alt,
              const int64_t *site_block, const int32_t *site_sigma, double clip, int64_t *out_block, double *out_llr,
              int64_t *out_sites) {
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
  return nvk_timed(ctx, NVK_K_ALLELE, [&] {
    hipLaunchKernelGGL(kernel, dim3(grid_of(n_reads, NT)), dim3(NT), 0, ctx->stream, n_reads, n_sites, alphabet,
                       ref_off, chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma, clip,
                       out_block, out_llr, out_sites);
  });
}

}  // namespace

extern "C" int nvk_phase_links_dev(nvk_ctx *ctx, int64_t n_sites, int alphabet, const int64_t *site_lo,
                                   const int64_t *site_hi, const int32_t *site_alt, const int32_t *chain,
                                   const int64_t *row_read, const double *val, double clip, double *out_link,
                                   int64_t *out_shared) {
  return phase_links("nvk_phase_links_dev", ctx, n_sites, 1, alphabet, site_lo, site_hi, site_alt, chain, nullptr,
                     row_read, val, clip, out_link, out_shared);
}

extern "C" int nvk_phase_span_links_dev(nvk_ctx *ctx, int64_t n_sites, int span, int alphabet, const int64_t *site_lo,
                                        const int64_t *site_hi, const int32_t *site_alt, const int64_t *site_first,
                                        const int64_t *row_read, const double *val, double clip, double *out_link,
                                        int64_t *out_shared) {
  return phase_links("nvk_phase_span_links_dev", ctx, n_sites, span, alphabet, site_lo, site_hi, site_alt, nullptr,
                     site_first, row_read, val, clip, out_link, out_shared);
}

extern "C" int nvk_phase_tag_dev(nvk_ctx *ctx, int64_t n_reads, int64_t n_sites, int alphabet, const int64_t *ref_off,
                                 const int64_t *chunk_start, const int32_t *reverse, const int64_t *key,
                                 const double *val, const int64_t *site_pos, const int32_t *site_alt,
                                 const int64_t *site_block, const int32_t *site_sigma, double clip,
                                 int64_t *out_block, double *out_llr, int64_t *out_sites) {
  return phase_tag("nvk_phase_tag_dev", phase_tag_kernel, ctx, n_reads, n_sites, alphabet, ref_off, chunk_start,
                   reverse, key, val, site_pos, site_alt, site_block, site_sigma, clip, out_block, out_llr, out_sites);
}

extern "C" int nvk_phase_tag_blocks_dev(nvk_ctx *ctx, int64_t n_reads, int64_t n_sites, int alphabet,
                                        const int64_t *ref_off, const int64_t *chunk_start, const int32_t *reverse,
                                        const int64_t *key, const double *val, const int64_t *site_pos,
                                        const int32_t *site_alt, const int64_t *site_block, const int32_t *site_sigma,
                                        double clip, int64_t *out_block, double *out_llr, int64_t *out_sites) {
  return phase_tag("nvk_phase_tag_blocks_dev", phase_tag_blocks_kernel, ctx, n_reads, n_sites, alphabet, ref_off,
                   chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma, clip, out_block, out_llr,
                   out_sites);
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
  return nvk_timed(ctx, NVK_K_ALLELE, [&] {
    hipLaunchKernelGGL(phase_votes_kernel, dim3(grid_of(n_sites, NT / 64)), dim3(NT), 0, ctx->stream, n_sites,
                       alphabet, site_lo, site_hi, site_alt, site_block, site_sigma, row_read, val, read_block,
                       read_llr, clip, out_vote, out_agree, out_against);
  });
}
