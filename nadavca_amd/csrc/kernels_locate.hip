// Signal location for signal_locate_batch (nadavca_amd/locate.py): a dense subsequence alignment of every query (a
// chunk of a read's events) against every column of every target (the k-mer levels of a contig on one strand).  The
// rules are those of include/nadavca_hip.h (nvk_signal_locate_dev); the CPU restatement the tests hold this kernel to
// is tests/host_shims/locate_host.cpp, which sweeps the full matrix without tiles.
//
// Every move consumes one event, so S(i, j) depends on the columns [j - 2 i, j] alone: a path over Q events spans at
// most 2 Q - 1 columns.  A target is therefore cut into tiles of T = 64 CPL columns of which the first H = T - V are
// halo (H >= 2 (max_events - 1)) and the last V are valid: the valid columns' cells are exactly the full matrix's, for
// any cut.  V is a multiple of the block width 256, so a tile owns whole blocks of the output.
//
// One wave64 per (query, tile), one block per wave.  Lane l owns the CPL contiguous columns l CPL .. l CPL + CPL - 1 of
// the tile: their mu / ac / mc, the row's S, the carried (start column, first event) and the column's running best
// end, all in registers.  A row is updated in place from the lane's last column down, so the neighbours j - 1 and
// j - 2 are still the previous row's; at a lane's first two columns they are the previous lane's last two, taken by a
// DPP wave rotate before the update (lane 0 takes -inf: the tile's left edge is a target's edge or halo).  The loop
// over the events is wave-uniform: the event's level, the open candidate and the end's trim are scalars.  No LDS, no
// atomics, no traceback: the carried start makes the walk back unnecessary.
//
// The kernel adds, multiplies and compares doubles and nothing else: with -ffp-contract=off every score is the rounded
// operation the contract writes, on the device as on the host.
#include <vector>

#include "kmer_hmm.h"
#include "nvk_internal.h"
#include "wave.h"

namespace {

constexpr int LOC_MAX_TARGET = 1 << 30;  // columns per target: keeps every column index inside int32

struct LocTile {
  int64_t flat0;  // index of the tile's column 0 in mu / ac / mc (before the target's first column in its first tile)
  int32_t t0;     // that column inside the target (negative in a target's first tile)
  int32_t L;      // the target's columns
  int32_t blk0;   // the first block of the tile's valid columns, in the numbering over all targets
  int32_t nblk;   // blocks the tile owns
};

struct LocateArgs {
  const double *level;  // the events' levels, query q at q_off[q]
  const int64_t *q_off;
  const double *mu, *ac, *mc;
  const LocTile *tiles;
  int64_t n_tiles, n_blocks;
  int64_t q0;           // the launch's first query
  double l_stay, l_step, l_skip, trim_cost;
  double *out_score;
  int32_t *out_hit;
};

// CPL columns per lane: a tile of T = 64 CPL columns, the last V of them valid
template <int CPL, int V>
__global__ __launch_bounds__(64) void locate_kernel(LocateArgs a) {
  constexpr int T = 64 * CPL, H = T - V, G = NVK_LOC_BLOCK / CPL;  // G: lanes per block of the output
  static_assert(V % NVK_LOC_BLOCK == 0 && H % CPL == 0 && (H / CPL) % G == 0, "blocks start at lane groups");
  const double NINF = nvk_neg_inf();
  const int lane = threadIdx.x;
  const int64_t id = blockIdx.x;
  const int64_t q = a.q0 + id / a.n_tiles;
  const LocTile tile = a.tiles[id % a.n_tiles];
  const int64_t e0 = a.q_off[q];
  const int Q = __builtin_amdgcn_readfirstlane((int)(a.q_off[q + 1] - e0));
  const double *lev = a.level + e0;
  const double l_stay = a.l_stay, l_step = a.l_step, l_skip = a.l_skip, trim = a.trim_cost;

  double mu[CPL], ac[CPL], mc[CPL], S[CPL], best[CPL];
  int src[CPL], bpk[CPL];  // src: (start column inside the tile) << 8 | first event; bpk: last event << 20 | src
#pragma unroll
  for (int c = 0; c < CPL; c++) {
    const int t = lane * CPL + c, j = tile.t0 + t;
    const bool inside = j >= 0 && j < tile.L;
    // a column outside the target emits -inf: its cells are -inf in every row and feed nothing
    mu[c] = inside ? a.mu[tile.flat0 + t] : 0.0;
    ac[c] = inside ? a.ac[tile.flat0 + t] : NINF;
    mc[c] = inside ? a.mc[tile.flat0 + t] : 0.0;
    S[c] = best[c] = NINF;
    src[c] = 0;
    bpk[c] = -1;
  }
  for (int i = 0; i < Q; i++) {
    const double e = lev[i];
    const double open = (double)i * trim, tail = (double)(Q - 1 - i) * trim;
    // the previous lane's last two columns of the previous row
    double p1 = dpp_ror1(S[CPL - 1]), p2 = dpp_ror1(S[CPL - 2]);
    const int q1 = dpp_ror1(src[CPL - 1]), q2 = dpp_ror1(src[CPL - 2]);
    if (lane == 0) p1 = p2 = NINF;
#pragma unroll
    for (int c = CPL - 1; c >= 0; c--) {
      const double s1 = c >= 1 ? S[c >= 1 ? c - 1 : 0] : p1;
      const double s2 = c >= 2 ? S[c >= 2 ? c - 2 : 0] : (c == 1 ? p1 : p2);
      const int r1 = c >= 1 ? src[c >= 1 ? c - 1 : 0] : q1;
      const int r2 = c >= 2 ? src[c >= 2 ? c - 2 : 0] : (c == 1 ? q1 : q2);
      const double em = gauss_log(e, mu[c], ac[c], mc[c]);
      double v = open;
      int s = ((lane * CPL + c) << 8) | i;
      const double step = s1 + l_step, stay = S[c] + l_stay, skip = s2 + l_skip;
      if (step > v) {
        v = step;
        s = r1;
      }
      if (stay > v) {
        v = stay;
        s = src[c];
      }
      if (skip > v) {
        v = skip;
        s = r2;
      }
      S[c] = v + em;
      src[c] = s;
      const double end = S[c] + tail;
      if (end > best[c]) {
        best[c] = end;
        bpk[c] = (i << 20) | s;
      }
    }
  }
  // the lane's best column, then the block's over its G lanes: the largest end, the smallest column among equal ones
  double lb = NINF;
  int lpk = -1, lcol = 0x7fffffff;
#pragma unroll
  for (int c = 0; c < CPL; c++)
    if (best[c] > lb) {
      lb = best[c];
      lpk = bpk[c];
      lcol = lane * CPL + c;
    }
  for (int off = G / 2; off; off >>= 1) {
    const double ob = __shfl_xor(lb, off);
    const int opk = __shfl_xor(lpk, off), ocol = __shfl_xor(lcol, off);
    if (ob > lb || (ob == lb && ocol < lcol)) {
      lb = ob;
      lpk = opk;
      lcol = ocol;
    }
  }
  const int b = (lane - H / CPL) / G;
  if (lane >= H / CPL && lane % G == 0 && b < tile.nblk) {
    const int64_t o = q * a.n_blocks + tile.blk0 + b;
    a.out_score[o] = lb;
    int4 hit = make_int4(-1, -1, -1, -1);
    if (lpk >= 0) hit = make_int4(tile.t0 + lcol, lpk >> 20, tile.t0 + ((lpk & 0xfffff) >> 8), lpk & 0xff);
    *(int4 *)(a.out_hit + 4 * o) = hit;
  }
}

}  // namespace

extern "C" int nvk_signal_locate_dev(nvk_ctx *ctx, int64_t n_queries, int64_t total_events, const double *level,
                                     const int64_t *q_off, int64_t n_targets, int64_t total_cols, const double *mu,
                                     const double *ac, const double *mc, const int64_t *col_off, int max_events,
                                     double l_stay, double l_step, double l_skip, double trim_cost, int64_t n_blocks,
                                     double *out_score, int32_t *out_hit) {
  const char *what = "nvk_signal_locate_dev";
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_queries < 0 || n_queries > 0x7fffffff || n_targets < 0 || n_targets > 0x7fffffff || total_events < 0 ||
      total_cols < 0 || n_blocks < 0) {
    nvk_set_error("%s: n_queries %lld, n_targets %lld, total_events %lld, total_cols %lld or n_blocks %lld out of range",
                  what, (long long)n_queries, (long long)n_targets, (long long)total_events, (long long)total_cols,
                  (long long)n_blocks);
    return NVK_ERR_INVALID;
  }
  if (max_events < 1) {
    nvk_set_error("%s: max_events %d is below 1", what, max_events);
    return NVK_ERR_INVALID;
  }
  if (max_events > NVK_LOC_MAX_EVENTS) {
    nvk_set_error("%s: max_events %d is above %d", what, max_events, (int)NVK_LOC_MAX_EVENTS);
    return NVK_ERR_UNSUPPORTED;
  }
  if (int rc = check_log_costs(what, "l_stay %g, l_step %g, l_skip %g or trim_cost %g",
                               {l_stay, l_step, l_skip, trim_cost}))
    return rc;
  if (!q_off || !col_off || (total_events > 0 && !level) || (total_cols > 0 && (!mu || !ac || !mc))) {
    nvk_set_error("%s: NULL levels, offsets or column tables", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> qoff, coff;
  int rc = nvk_fetch_offsets(ctx, "query", q_off, n_queries, qoff, "total_events", total_events);
  if (rc) return rc;
  if ((rc = nvk_fetch_offsets(ctx, "column", col_off, n_targets, coff, "total_cols", total_cols))) return rc;
  for (int64_t q = 0; q < n_queries; q++)
    if (qoff[q + 1] - qoff[q] > max_events) {
      nvk_set_error("%s: query %lld has %lld events, above max_events %d", what, (long long)q,
                    (long long)(qoff[q + 1] - qoff[q]), max_events);
      return NVK_ERR_INVALID;
    }
  int64_t blocks = 0;
  for (int64_t t = 0; t < n_targets; t++) {
    const int64_t L = coff[t + 1] - coff[t];
    if (L > LOC_MAX_TARGET) {
      nvk_set_error("%s: target %lld has %lld columns, above %d", what, (long long)t, (long long)L, LOC_MAX_TARGET);
      return NVK_ERR_INVALID;
    }
    blocks += (L + NVK_LOC_BLOCK - 1) / NVK_LOC_BLOCK;
  }
  if (blocks != n_blocks || blocks > 0x7fffffff) {
    nvk_set_error("%s: n_blocks %lld, the targets have %lld blocks of %d columns", what, (long long)n_blocks,
                  (long long)blocks, (int)NVK_LOC_BLOCK);
    return NVK_ERR_INVALID;
  }
  if (n_queries == 0 || n_targets == 0 || n_blocks == 0) return NVK_OK;
  if (!out_score || !out_hit) {
    nvk_set_error("%s: NULL output", what);
    return NVK_ERR_INVALID;
  }
  // the tiles: T = 1024 columns, of which V = 768 are valid for up to 128 events (halo 256 >= 254) and V = 512 for up
  // to 256 (halo 512 >= 510)
  const bool wide = max_events > 128;
  const int64_t V = wide ? 512 : 768, H = 1024 - V, per = V / NVK_LOC_BLOCK;
  std::vector<LocTile> tiles;
  int64_t blk0 = 0;
  for (int64_t t = 0; t < n_targets; t++) {
    const int64_t L = coff[t + 1] - coff[t], nb = (L + NVK_LOC_BLOCK - 1) / NVK_LOC_BLOCK;
    for (int64_t k = 0; k * V < L; k++) {
      LocTile x;
      x.t0 = (int32_t)(k * V - H);
      x.flat0 = coff[t] + x.t0;
      x.L = (int32_t)L;
      x.blk0 = (int32_t)(blk0 + k * per);
      x.nblk = (int32_t)(nb - k * per < per ? nb - k * per : per);
      tiles.push_back(x);
    }
    blk0 += nb;
  }
  const int64_t n_tiles = (int64_t)tiles.size();
  // (the seed aligner's offsets workspace serves: the two never run at once on a context)
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_OFF, tiles.size() * sizeof(LocTile) + 64))) return rc;
  NVK_HIP(hipMemcpyAsync(ctx->ws[WS_SEED_OFF], tiles.data(), tiles.size() * sizeof(LocTile), hipMemcpyHostToDevice,
                         ctx->stream));
  LocateArgs a;
  a.level = level;
  a.q_off = q_off;
  a.mu = mu;
  a.ac = ac;
  a.mc = mc;
  a.tiles = (const LocTile *)ctx->ws[WS_SEED_OFF];
  a.n_tiles = n_tiles;
  a.n_blocks = n_blocks;
  a.l_stay = l_stay;
  a.l_step = l_step;
  a.l_skip = l_skip;
  a.trim_cost = trim_cost;
  a.out_score = out_score;
  a.out_hit = out_hit;
  // one wave per (query, tile); a launch takes as many queries as keep its grid inside 2^30 blocks
  const int64_t q_per = (int64_t)(1 << 30) / n_tiles > 0 ? (int64_t)(1 << 30) / n_tiles : 1;
  for (int64_t q0 = 0; q0 < n_queries; q0 += q_per) {
    const int64_t nq = n_queries - q0 < q_per ? n_queries - q0 : q_per;
    a.q0 = q0;
    const dim3 grid((unsigned)(nq * n_tiles));
    if (wide)
      hipLaunchKernelGGL((locate_kernel<16, 512>), grid, dim3(64), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL((locate_kernel<16, 768>), grid, dim3(64), 0, ctx->stream, a);
    NVK_HIP(hipGetLastError());
  }
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
