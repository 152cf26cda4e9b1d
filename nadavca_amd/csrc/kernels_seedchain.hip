// Chaining stage of the seed aligner (nadavca_amd/seedalign.py, chain=1): per read, the best collinear chain of its
// seeds and, from the chain's anchors, the band centre of every strip of 64 read rows, which
// nvk_seed_extend_path_dev (kernels_seedext.hip) then follows.  The rules are those of include/nadavca_hip.h
// (nvk_seed_chain_dev), integers only; the CPU restatement the tests hold this kernel to is
// tests/host_shims/seedchain_host.cpp.
//
// One wave64 per read; a persistent grid takes reads from an atomic counter; control flow is wave-uniform.  The
// seeds arrive sorted by (p, i) and are scored in that order.  The last 64 of them, (i, p, f), live one per lane,
// lane l holding seed t - 1 - l: every lane scores the new seed against its own, a wave maximum picks the best score
// and a ballot the nearest lane that reaches it (score and lane do not pack into one int32: f goes up to 2^30), then
// the ring rotates by one lane and lane 0 takes the new seed.  Seeds are loaded 64 at a time, coalesced, and read
// out by lane; (f, pred) of a block of 64 collect in the lanes and go to the workspace in one store.  The backtrack
// is walked by every lane alike: an anchor a with its neighbours a- and a+ on the chain is the nearest anchor of the
// strip centres c with i(a-) + i(a) < 2 c <= i(a) + i(a+), a run of strips that the lanes write together.
#include <vector>

#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int CHAIN_WMAX = 256;            // as the extension's band
constexpr int CHAIN_MAX_READ = 1 << 26;    // as the extension's
constexpr int CHAIN_MAX_SEEDS = 1 << 26;   // per read: keeps f <= 2^26 * k (k <= 16) inside int32

struct ChainArgs {
  const int64_t *q_off;
  const int32_t *strand;
  const int64_t *seed_off;
  const int32_t *seed_i, *seed_p;
  int k, w, max_gap, lookback;
  const int64_t *strip_off;
  int32_t *strip_diag;
  int32_t *out_chain;  // 2 per read: chain score, anchors
  int2 *fp;            // workspace, per seed: (f, pred), pred counted from the read's first seed
  int n_reads;
  int *counter;
};

__global__ __launch_bounds__(64) void seedchain_kernel(ChainArgs a) {
  const int lane = threadIdx.x;
  for (;;) {
    // (every lane takes part in the atomic: kernels_seedext.hip says why)
    const int rd = __builtin_amdgcn_readfirstlane(atomicAdd(a.counter, lane == 0 ? 1 : 0));
    if (rd >= a.n_reads) return;
    const int64_t s0 = uniform64(a.seed_off[rd]);
    const int st = __builtin_amdgcn_readfirstlane(a.strand[rd]);
    const int n = st == 0 || st == 1 ? (int)(uniform64(a.seed_off[rd + 1]) - s0) : 0;
    const int m = (int)(uniform64(a.q_off[rd + 1]) - uniform64(a.q_off[rd]));
    int ri = 0, rp = 0, rf = 0;        // the ring: seed t - 1 - lane
    int blk_i = 0, blk_p = 0;          // seed (t & ~63) + lane
    int of = 0, op = -1;               // (f, pred) of seed (t & ~63) + lane, once scored
    int bf = 0, bt = -1;               // the chain's end: largest f, then smallest t
    __syncthreads();                   // (the previous read's last loads of fp, should the two share seeds' slots)
    for (int t = 0; t < n; t++) {
      const int x = t & 63;
      if (x == 0) {
        blk_i = t + lane < n ? a.seed_i[s0 + t + lane] : 0;
        blk_p = t + lane < n ? a.seed_p[s0 + t + lane] : 0;
      }
      const int ci = __builtin_amdgcn_readlane(blk_i, x), cp = __builtin_amdgcn_readlane(blk_p, x);
      const int di = ci - ri, dp = cp - rp, gap = dp > di ? dp - di : di - dp;
      const bool ok = lane < min(t, a.lookback) && di > 0 && di <= a.max_gap && dp > 0 && dp <= a.max_gap &&
                      gap <= a.w;
      const int cand = ok ? rf + min(min(di, dp), a.k) - gap : 0;
      const int best = __builtin_amdgcn_readfirstlane(wave_max(cand));
      int f = a.k, pred = -1;
      if (best > a.k) {  // (k >= 1: a lane without a candidate, at 0, is never the winner)
        f = best;
        pred = t - 1 - (int)__builtin_ctzll(__ballot(cand == best));  // the nearest predecessor: the lowest lane
      }
      if (lane == x) {
        of = f;
        op = pred;
      }
      if (x == 63 || t == n - 1)
        if (lane <= x) a.fp[s0 + t - x + lane] = make_int2(of, op);
      if (f > bf) {
        bf = f;
        bt = t;
      }
      ri = dpp_ror1(ri);
      rp = dpp_ror1(rp);
      rf = dpp_ror1(rf);
      if (lane == 0) {
        ri = ci;
        rp = cp;
        rf = f;
      }
    }
    __syncthreads();  // every lane's fp stores before the walk reads them
    int cnt = 0;
    if (bt >= 0) {
      const int64_t so = uniform64(a.strip_off[rd]);
      int t = bt, hi = (m + 63) / 64 - 1;  // hi: the last strip the anchor at t may take
      int ia = __builtin_amdgcn_readfirstlane(a.seed_i[s0 + t]), pa = __builtin_amdgcn_readfirstlane(a.seed_p[s0 + t]);
      for (;;) {
        cnt++;
        const int u = __builtin_amdgcn_readfirstlane(a.fp[s0 + t].y);
        int iu = 0, pu = 0, lo = 0;
        if (u >= 0) {
          iu = __builtin_amdgcn_readfirstlane(a.seed_i[s0 + u]);
          pu = __builtin_amdgcn_readfirstlane(a.seed_p[s0 + u]);
          lo = max(((ia + iu - 64) >> 7) + 1, 0);  // the first strip s with 2 (64 s + 32) > i(a) + i(a-)
        }
        for (int s = lo + lane; s <= hi; s += 64) a.strip_diag[so + s] = pa - ia;
        if (u < 0 || cnt >= n) break;  // (a chain has at most n anchors: the guard holds the walk to that regardless)
        hi = min(hi, lo - 1);
        t = u;
        ia = iu;
        pa = pu;
      }
    }
    if (lane == 0) *(int2 *)(a.out_chain + 2 * (int64_t)rd) = make_int2(bf, cnt);
  }
}

}  // namespace

extern "C" int nvk_seed_chain_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int64_t *q_off,
                                  const int32_t *strand, int64_t total_seeds, const int64_t *seed_off,
                                  const int32_t *seed_i, const int32_t *seed_p, int k, int band, int max_gap,
                                  int lookback, int64_t total_strips, const int64_t *strip_off, int32_t *strip_diag,
                                  int32_t *out_chain) {
  const char *what = "nvk_seed_chain_dev";
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff || total_query < 0 || total_seeds < 0 || total_strips < 0) {
    nvk_set_error("%s: n_reads %lld, total_query %lld, total_seeds %lld or total_strips %lld out of range", what,
                  (long long)n_reads, (long long)total_query, (long long)total_seeds, (long long)total_strips);
    return NVK_ERR_INVALID;
  }
  if (band > CHAIN_WMAX) {
    nvk_set_error("%s: band %d is above the compiled limit %d", what, band, CHAIN_WMAX);
    return NVK_ERR_UNSUPPORTED;
  }
  if (k < 1 || k > 16 || band < 1 || max_gap < 1 || max_gap > CHAIN_MAX_READ || lookback < 1 || lookback > 64) {
    nvk_set_error("%s: k %d, band %d, max_gap %d or lookback %d out of range", what, k, band, max_gap, lookback);
    return NVK_ERR_INVALID;
  }
  if (!q_off || !seed_off || !strip_off || (total_seeds > 0 && (!seed_i || !seed_p)) ||
      (total_strips > 0 && !strip_diag)) {
    nvk_set_error("%s: NULL offsets, seeds or strip centres", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off, soff, toff;
  int rc = nvk_fetch_offsets(ctx, "query", q_off, n_reads, off, "total_query", total_query);
  if (rc) return rc;
  if ((rc = nvk_fetch_offsets(ctx, "seed", seed_off, n_reads, soff, "total_seeds", total_seeds))) return rc;
  if ((rc = nvk_fetch_offsets(ctx, "strip", strip_off, n_reads, toff, "total_strips", total_strips))) return rc;
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t m = off[r + 1] - off[r];
    if (m > CHAIN_MAX_READ || soff[r + 1] - soff[r] > CHAIN_MAX_SEEDS) {
      nvk_set_error("%s: read %lld has %lld bases or %lld seeds, above %d", what, (long long)r, (long long)m,
                    (long long)(soff[r + 1] - soff[r]), CHAIN_MAX_READ);
      return NVK_ERR_INVALID;
    }
    if (toff[r + 1] - toff[r] != (m + 63) / 64) {
      nvk_set_error("%s: read %lld of %lld bases has %lld strips, not %lld", what, (long long)r, (long long)m,
                    (long long)(toff[r + 1] - toff[r]), (long long)((m + 63) / 64));
      return NVK_ERR_INVALID;
    }
  }
  if (n_reads == 0) return NVK_OK;
  if (!strand || !out_chain) {
    nvk_set_error("%s: NULL strand or output", what);
    return NVK_ERR_INVALID;
  }
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_CHAIN, 64 + (size_t)total_seeds * sizeof(int2)))) return rc;
  ChainArgs a;
  a.q_off = q_off;
  a.strand = strand;
  a.seed_off = seed_off;
  a.seed_i = seed_i;
  a.seed_p = seed_p;
  a.k = k;
  a.w = band;
  a.max_gap = max_gap;
  a.lookback = lookback;
  a.strip_off = strip_off;
  a.strip_diag = strip_diag;
  a.out_chain = out_chain;
  a.counter = (int *)ctx->ws[WS_SEED_CHAIN];
  a.fp = (int2 *)((char *)ctx->ws[WS_SEED_CHAIN] + 64);
  a.n_reads = (int)n_reads;
  {
    TimerScope ts(ctx, NVK_K_SEED);
    const int64_t resident = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 16;
    NVK_HIP(hipMemsetAsync(a.counter, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(seedchain_kernel, dim3((unsigned)(n_reads < resident ? n_reads : resident)), dim3(64), 0,
                       ctx->stream, a);
    NVK_HIP(hipGetLastError());
  }
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
