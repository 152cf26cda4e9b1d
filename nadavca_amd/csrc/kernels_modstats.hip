// The M-step of modified-base table training (nadavca_amd/mod_train.py: estimate_mod_model): weighted per-k-mer sample
// statistics over the final events of an aligned batch, every event counted under each modification state of the sites
// in its k-mer window with the probability of that state (the contract: include/nadavca_hip.h, nvk_mod_kmer_rows_dev).
//
//   nvk_mod_kmer_rows_dev     per (read, base) with 1 .. 4 sites in its window: one row per non-empty subset of them,
//                             (key, w, n, sd, sq): the subset's k-mer, its probability, the event's sample count and
//                             its sums of deviations and squared deviations from the k-mer's current level.  Two calls:
//                             the first counts the rows per base, the second fills them.
//   nvk_mod_kmer_reduce_dev   per run of equal keys in stable key order (the caller sorts and gathers: plumbing): the
//                             weighted sums W, Nw, Sd, Sq and the run's row count
//
// No floating-point atomics: an event's two sums are one thread's ascending loop, a subset's values follow from them by
// a handful of rounded operations, and a key's sums are a lane's loop over its rows followed by a butterfly over the
// wave (wave_sum_n, the order of nvk_site_moments_dev).  Two runs give the same bits, and the numpy restatement of the tests
// gives them too.
//
// Work split of the row pass: one wave per read, its lanes over the read's bases (read_rows.h); the base pointers of
// the read's site list are wave-uniform with the rest of its view.  A lane finds the sites of its window
// by a binary search over the read's site positions (a read holds tens of sites; neighbouring lanes walk the same few
// cache lines) and reads at most five entries from there.  An event's samples are read once, whatever the number of
// rows: a and b are sums around the canonical window's level c0, and the sums around another level c follow from
// d = c0 - c without the samples.  Only bases near a site do any of this; the others cost the search.  The pass moves
// 8 B per sample of the events it counts in, and 40 B per row out.
//
// Work split of the reduction: ONE WAVE PER RUN (grid-stride), lane l over the run's rows l, l + 64, ..., the four sums
// side by side.  A 5^6 table has a few thousand runs with M in them; a run of c rows keeps min(c, 64) lanes busy.
//
// Resources on gfx950: no LDS, no scratch.
#include <math.h>

#include <vector>

#include "nvk_internal.h"
#include "kmer.h"
#include "read_rows.h"
#include "wave.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_SITES = 4; // sites of one window at most: 2^4 - 1 rows
constexpr int NCOL = 4;      // w, n, sd, sq

// the row pass of read_rows.h.  FILL false: out_count per base; true: the rows.  A read that did not align has its
// rows counted and written with key -1.
// info[0]: the bases with more than MAX_SITES sites in their window; info[1]: set where row_off disagrees.
template <bool FILL>
__global__ __launch_bounds__(NT) void mod_rows_kernel(int64_t n_reads, ReadArrays arrays, const int32_t *events,
                                                      const int32_t *reference, int k, int central, int alphabet,
                                                      int trim, const int64_t *site_off, const int32_t *site_pos,
                                                      const double *site_gamma, int mod_code, const double *level,
                                                      int64_t n_rows, const int64_t *row_off, int64_t *out_count,
                                                      int64_t *out_key, double *out_val, unsigned long long *info) {
  const DeviceModel dm{k, central, alphabet, 0, nullptr, nullptr, nullptr};  // (kmer.h reads the window's shape only)
  int skipped = 0;
  for_each_read<int, RV_SIGNAL | RV_CONTEXTS>(arrays, n_reads, [&](const ReadView<int> &v) {
    const int64_t r0 = v.r0;
    const int R = v.R;
    const int S = (int)(site_off[v.rd + 1] - site_off[v.rd]);
    const int32_t *sp = site_pos + site_off[v.rd];
    const double *sg = site_gamma + site_off[v.rd];
    const int32_t *ref = reference + r0;
    for_each_base(v, [&](int g) {
      const int p0 = g - central;  // first base of the window, reference-part coordinates
      // the read's sites inside [p0, p0 + k): the first MAX_SITES of them, and whether there is one more
      int lo = 0, hi = S;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sp[mid] < p0) lo = mid + 1; else hi = mid;
      }
      // (a position outside the window or the read ends the walk: sorted positions inside [0, R) never do so early, and
      // anything else stays inside the site list and the reference part)
      auto inside = [&](int i, int &q) {
        if (i >= S) return false;
        q = sp[i];
        return q >= p0 && q < p0 + k && q >= 0 && q < R;
      };
      int m = 0, sh[MAX_SITES];
      double gm[MAX_SITES];
      bool open = true;
#pragma unroll
      for (int t = 0; t < MAX_SITES; t++) {
        int q = 0;
        open = open && inside(lo + t, q);
        sh[t] = open ? q - p0 : 0;
        gm[t] = open ? sg[lo + t] : 0.0;
        if (open) m = t + 1;
      }
      int q5 = 0;
      const bool over = open && inside(lo + MAX_SITES, q5);
      if (over) skipped++;
      const int cnt = over ? 0 : (1 << m) - 1;
      if (!FILL) {
        out_count[r0 + g] = cnt;
        return;
      }
      const int64_t row0 = row_off[r0 + g], row1 = row_off[r0 + g + 1];
      if (row0 < 0 || row1 > n_rows || row1 - row0 != cnt) {  // the caller's width is not this pass's: write nothing
        atomicOr(info + 1, 1ull);
        return;
      }
      if (cnt == 0) return;
      // the event, counted under kmer_event_kernel's conditions: its sums around the canonical window's level
      int64_t key0 = -1;
      int len = 0;
      double c0 = 0.0, a = 0.0, b = 0.0;
      if (v.live && counted_base(g, R, trim) && window_inside(g, k, central, R, v.B, v.A)) {
        int s, e;
        event_span(events, r0 + g, v.N, s, e);
        if (e > s) key0 = kmer_id_checked(dm, ref, R, v.cb, v.B, v.ca, v.A, g);
        if (key0 >= 0) {
          len = e - s;
          c0 = level[key0];
          for (int i = s; i < e; i++) {
            const double dv = v.x[i] - c0;
            a = a + dv;
            b = b + dv * dv;
          }
        }
      }
      // what a site adds to the key when it is modified: (mod_code - its base) * alphabet^(k - 1 - its place)
      int64_t delta[MAX_SITES];
#pragma unroll
      for (int t = 0; t < MAX_SITES; t++) {
        int64_t pw = 1;
        for (int i = sh[t] + 1; i < k; i++) pw *= alphabet;
        delta[t] = t < m ? (int64_t)(mod_code - ref[p0 + sh[t]]) * pw : 0;
      }
      const double n = (double)len;
      for (int mask = 1; mask <= cnt; mask++) {
        int64_t key = -1;
        double w = 0.0, sd = 0.0, sq = 0.0;
        if (key0 >= 0) {
          key = key0;
          w = 1.0;
#pragma unroll
          for (int t = 0; t < MAX_SITES; t++) {
            if (t < m) {
              if ((mask >> t) & 1) {
                key += delta[t];
                w = w * gm[t];
              } else {
                w = w * (1.0 - gm[t]);
              }
            }
          }
          const double d = c0 - level[key];
          sd = a + n * d;
          sq = b + (2.0 * d) * a + (n * d) * d;
        }
        const int64_t row = row0 + mask - 1;
        out_key[row] = key;
        double *dst = out_val + (size_t)row * NCOL;
        dst[0] = w;
        dst[1] = n;
        dst[2] = sd;
        dst[3] = sq;
      }
    });
  });
  skipped = wave_sum(skipped);
  if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(info, (unsigned long long)skipped);
}

// one wave per run (grid-stride): the four weighted sums of its rows and their number
__global__ __launch_bounds__(NT) void mod_reduce_kernel(int64_t n_keys, const double *val, const int64_t *run_off,
                                                        double *out_sum, int64_t *out_rows) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (NT / 64);
  for (int64_t q = (int64_t)blockIdx.x * (NT / 64) + wave; q < n_keys; q += waves) {
    const int64_t lo = run_off[q], hi = run_off[q + 1];
    double p[NCOL] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = lo + lane; i < hi; i += 64) {
      const double *v = val + (size_t)i * NCOL;
      const double w = v[0];
      p[0] = p[0] + w;
      p[1] = p[1] + w * v[1];
      p[2] = p[2] + w * v[2];
      p[3] = p[3] + w * v[3];
    }
    wave_sum_n(p);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < NCOL; c++) out_sum[(size_t)q * NCOL + c] = p[c];
      out_rows[q] = hi - lo;
    }
  }
}

}  // namespace

extern "C" int nvk_mod_kmer_rows_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const double *signal,
                                     const int64_t *sig_off, const int32_t *events, const int64_t *ref_off,
                                     const int32_t *reference, const int32_t *ctx_before, const int64_t *cb_off,
                                     const int32_t *ctx_after, const int64_t *ca_off, const int32_t *status, int k,
                                     int central, int alphabet, int trim, int64_t n_sites, const int64_t *site_off,
                                     const int32_t *site_pos, const double *site_gamma, int mod_code,
                                     const double *level, int64_t n_rows, const int64_t *row_off, int64_t *out_count,
                                     int64_t *out_key, double *out_val, int64_t *windows_skipped) {
  const char *what = "nvk_mod_kmer_rows_dev";
  if (windows_skipped) *windows_skipped = 0;
  if (n_sites < 0 || n_rows < 0) {
    nvk_set_error("%s: invalid argument", what);
    return NVK_ERR_INVALID;
  }
  if (kmer_table_size(k, alphabet) < 0 || central < 0 || central >= k || trim < 0) {
    nvk_set_error("%s: k %d, central %d, alphabet %d, trim %d outside the served range (1 <= k, 0 <= central < k, "
                  "alphabet^k <= 2^31, trim >= 0)", what, k, central, alphabet, trim);
    return NVK_ERR_INVALID;
  }
  if (mod_code < 0 || mod_code >= alphabet) {
    nvk_set_error("%s: mod_code %d outside the alphabet of %d letters", what, mod_code, alphabet);
    return NVK_ERR_INVALID;
  }
  const bool fill = out_key || out_val;
  if (fill && (!out_key || !out_val || !row_off)) {
    nvk_set_error("%s: out_key, out_val and row_off go together", what);
    return NVK_ERR_INVALID;
  }
  bool nothing;
  int rc = check_read_rows(what, ctx, n_reads, total_ref, ref_off, {{"signal", sig_off, signal},
                           {"context_before", cb_off, ctx_before}, {"context_after", ca_off, ctx_after}}, &nothing);
  if (rc) return rc;
  if (n_reads == 0) {
    if (n_sites != 0 || (fill && n_rows != 0)) {
      nvk_set_error("%s: n_sites %lld, n_rows %lld with no reads", what, (long long)n_sites, (long long)n_rows);
      return NVK_ERR_INVALID;
    }
    return NVK_OK;
  }
  std::vector<int64_t> off;
  if ((rc = nvk_fetch_offsets(ctx, "site", site_off, n_reads, off, "n_sites", n_sites))) return rc;
  if (n_sites > 0 && (!site_pos || !site_gamma)) {
    nvk_set_error("%s: NULL site_pos or site_gamma", what);
    return NVK_ERR_INVALID;
  }
  if (nothing) {
    if (fill && n_rows != 0) {
      nvk_set_error("%s: n_rows %lld with no bases", what, (long long)n_rows);
      return NVK_ERR_INVALID;
    }
    return NVK_OK;
  }
  if (!reference || (!fill && !out_count) || (fill && (!events || !level))) {
    nvk_set_error("%s: NULL reference, events, level or output", what);
    return NVK_ERR_INVALID;
  }
  // two device counters behind the launchers' own in WS_MISC: every entry drains the stream before it returns
  if ((rc = nvk_ws_reserve(ctx, WS_MISC, 512))) return rc;
  unsigned long long *info = (unsigned long long *)((char *)ctx->ws[WS_MISC] + 256);
  NVK_HIP(hipMemsetAsync(info, 0, 2 * sizeof(unsigned long long), ctx->stream));
  {
    TimerScope ts(ctx, NVK_K_KMER);
    const ReadArrays arrays = {ref_off, status, nullptr, nullptr, signal, sig_off, ctx_before, cb_off, ctx_after,
                               ca_off};
    auto kernel = fill ? mod_rows_kernel<true> : mod_rows_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid_of(n_reads, NT / 64)), dim3(NT), 0, ctx->stream, n_reads, arrays, events,
                       reference, k, central, alphabet, trim, site_off, site_pos, site_gamma, mod_code, level, n_rows,
                       row_off, out_count, out_key, out_val, info);
  }
  NVK_HIP(hipGetLastError());
  unsigned long long h_info[2] = {0, 0};
  NVK_HIP(hipMemcpyAsync(h_info, info, sizeof(h_info), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  if (windows_skipped) *windows_skipped = (int64_t)h_info[0];
  if (h_info[1]) {
    nvk_set_error("%s: row_off does not hold this pass's row counts (or leaves 0 .. n_rows); no such base was written",
                  what);
    return NVK_ERR_INVALID;
  }
  return NVK_OK;
}

extern "C" int nvk_mod_kmer_reduce_dev(nvk_ctx *ctx, int64_t n_rows, int64_t n_keys, const double *val,
                                       const int64_t *run_off, double *out_sum, int64_t *out_rows) {
  const char *what = "nvk_mod_kmer_reduce_dev";
  if (!ctx || n_rows < 0 || n_keys < 0 || n_keys > ((int64_t)1 << 31)) {
    nvk_set_error("%s: invalid argument (0 <= n_keys <= 2^31, n_rows >= 0)", what);
    return NVK_ERR_INVALID;
  }
  if (n_keys == 0) return NVK_OK;
  if (!run_off || !out_sum || !out_rows || (n_rows > 0 && !val)) {
    nvk_set_error("%s: NULL input or output", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  // the runs: run_off[0] rows with a key < 0 come first, so the offsets start there and not at 0; brought to zero they
  // go through the one offsets check
  std::vector<int64_t> off((size_t)n_keys + 1);
  NVK_HIP(hipMemcpyAsync(off.data(), run_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t first = off[0];
  if (first < 0 || first > n_rows) {
    nvk_set_error("%s: run offsets start at %lld, outside 0 .. n_rows = %lld", what, (long long)first,
                  (long long)n_rows);
    return NVK_ERR_INVALID;
  }
  for (auto &o : off) o -= first;
  int rc = check_offsets("run", off.data(), n_keys);
  if (rc) return rc;
  if (off[(size_t)n_keys] != n_rows - first) {
    nvk_set_error("%s: run offsets end at %lld, n_rows is %lld", what, (long long)(off[(size_t)n_keys] + first),
                  (long long)n_rows);
    return NVK_ERR_INVALID;
  }
  return nvk_timed(ctx, NVK_K_KMER, [&] {
    hipLaunchKernelGGL(mod_reduce_kernel, dim3(grid_of(n_keys, NT / 64)), dim3(NT), 0, ctx->stream, n_keys, val,
                       run_off, out_sum, out_rows);
  });
}
