// Phasing across weak sites (nadavca_amd/phase.py, span > 1): the two floating-point steps that differ from
// kernels_phase.hip once a site may be joined to any of the `span` sites before it.  The contract is in
// include/nadavca_hip.h (nvk_phase_span_links_dev); the forest between them (device.phase_forest) is torch on the
// device, the votes are nvk_phase_votes_dev's, which serves any block array.
//
//   nvk_phase_span_links_dev   per site s and w = 1 .. span: the link and the shared reads of nvk_phase_links_dev taken
//                              between sites s - w and s
//   nvk_phase_tag_blocks_dev   per read: the block with the largest |H| over ALL of the read's sites in that block (a
//                              singleton may sit inside another block, so a block is no interval of sites)
//
// Sums as in kernels_phase.hip: a site's sum is a lane's loop over rows l, l + 64, ... in ascending order followed by
// wave_sum's butterfly (wave_sum_n: the same additions per column), a read's H is one thread's left-to-right sum.  No
// atomics; two runs give the same bits, and column w = 1 has the bits of nvk_phase_links_dev.
//
// Work split: ONE WAVE PER SITE (grid-stride) in the links kernel.  A lane loads its row's read index and its evidence
// at s ONCE and then finds the read among the rows of the W earlier sites by W binary searches that advance in
// lockstep: the W loads of a step are independent and in flight together, so a step costs one memory round trip for
// all columns.  The columns live in registers, indexed statically (a template on 2 / 4 / 8 columns, the surplus
// masked by an empty range).  ONE THREAD PER READ in the tag kernel, one pass over the read's sites per distinct block
// (ascending block index, found by the pass before); a read meets a handful of sites and site_block stays in cache.
//
// Resources on gfx950: no LDS, no scratch; the register counts are in DESIGN.md 4.8.
#include <math.h>

#include <vector>

#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int NT = 256;

// (as in kernels_phase.hip, whose object stays what it was)
// min(max(d, -clip), clip); -inf and a d that is not a number give -clip
__device__ __forceinline__ double clipped(double d, double clip) { return d > -clip ? (d < clip ? d : clip) : -clip; }

// log(exp(a) + exp(b))
__device__ __forceinline__ double lae(double a, double b) { return fmax(a, b) + log1p(exp(-fabs(a - b))); }

// one wave per site (grid-stride); W >= span columns, column w - 1 for the site s - w
template <int W>
__global__ __launch_bounds__(NT) void phase_span_links_kernel(int64_t n_sites, int span, int alpha,
                                                              const int64_t *site_lo, const int64_t *site_hi,
                                                              const int32_t *site_alt, const int64_t *site_first,
                                                              const int64_t *row_read, const double *val, double clip,
                                                              double *out_link, int64_t *out_shared) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t s = (int64_t)blockIdx.x * (NT / 64) + wave; s < n_sites; s += waves) {
    double acc[W];
    int count[W];
    // the rows of the earlier sites (wave-uniform); an empty range where the column is not served
    int64_t plo[W], pn[W];
    int a1[W];
    const int64_t first = site_first[s];
    bool any = false;
#pragma unroll
    for (int w = 0; w < W; w++) {
      acc[w] = 0.0;
      count[w] = 0;
      plo[w] = 0;
      pn[w] = 0;
      a1[w] = 0;
      const int64_t p = s - (w + 1);
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

// one thread per read (grid-stride)
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
      const int64_t c0 = chunk_start[i];
      const bool rev = reverse[i] != 0;
      const int64_t s0 = lower_bound(site_pos, 0, n_sites, c0);
      const int64_t s1 = lower_bound(site_pos, s0, n_sites - s0, c0 + R);
      // the read's row of site s where it has evidence there, -1 otherwise
      auto row_of = [&](int64_t s) -> int64_t {
        const int64_t P = site_pos[s];
        const int a = site_alt[s];
        if (P < c0 || P >= c0 + R || a < 0 || a >= alpha) return -1;
        // forward columns need no flip; the rows of a reverse read run backwards (as consensus_kernel)
        const int64_t row = r0 + (rev ? R - 1 - (P - c0) : P - c0);
        return key[row] == P ? row : -1;
      };
      // the blocks of the read in ascending index: every pass sums the block `cur` and finds the next one
      bool more = false;
      int64_t cur = 0;
      for (int64_t s = s0; s < s1; s++) {
        if (row_of(s) < 0) continue;
        const int64_t b = site_block[s];
        if (!more || b < cur) cur = b;
        more = true;
      }
      while (more) {
        bool has_next = false;
        int64_t next = 0, n = 0;
        double h = 0.0;
        for (int64_t s = s0; s < s1; s++) {
          const int64_t row = row_of(s);
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

// (as check_phase of kernels_phase.hip)
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

extern "C" int nvk_phase_span_links_dev(nvk_ctx *ctx, int64_t n_sites, int span, int alphabet, const int64_t *site_lo,
                                        const int64_t *site_hi, const int32_t *site_alt, const int64_t *site_first,
                                        const int64_t *row_read, const double *val, double clip, double *out_link,
                                        int64_t *out_shared) {
  const char *what = "nvk_phase_span_links_dev";
  int rc;
  if ((rc = check_phase(what, ctx, n_sites, alphabet, clip))) return rc;
  if (span < 1 || span > 8) {
    nvk_set_error("%s: span %d outside 1 .. 8", what, span);
    return NVK_ERR_INVALID;
  }
  if (n_sites == 0) return NVK_OK;
  if (!site_lo || !site_hi || !site_alt || !site_first || !row_read || !val || !out_link || !out_shared) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  {
    TimerScope ts(ctx, NVK_K_ALLELE);
    const dim3 grid(grid_of(n_sites, NT / 64)), block(NT);
#define NVK_SPAN_LINKS(W)                                                                                        \
  hipLaunchKernelGGL(phase_span_links_kernel<W>, grid, block, 0, ctx->stream, n_sites, span, alphabet, site_lo, \
                     site_hi, site_alt, site_first, row_read, val, clip, out_link, out_shared)
    if (span <= 2)
      NVK_SPAN_LINKS(2);
    else if (span <= 4)
      NVK_SPAN_LINKS(4);
    else
      NVK_SPAN_LINKS(8);
#undef NVK_SPAN_LINKS
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_phase_tag_blocks_dev(nvk_ctx *ctx, int64_t n_reads, int64_t n_sites, int alphabet,
                                        const int64_t *ref_off, const int64_t *chunk_start, const int32_t *reverse,
                                        const int64_t *key, const double *val, const int64_t *site_pos,
                                        const int32_t *site_alt, const int64_t *site_block, const int32_t *site_sigma,
                                        double clip, int64_t *out_block, double *out_llr, int64_t *out_sites) {
  const char *what = "nvk_phase_tag_blocks_dev";
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
    hipLaunchKernelGGL(phase_tag_blocks_kernel, dim3(grid_of(n_reads, NT)), dim3(NT), 0, ctx->stream, n_reads, n_sites,
                       alphabet, ref_off, chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma,
                       clip, out_block, out_llr, out_sites);
  }
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
