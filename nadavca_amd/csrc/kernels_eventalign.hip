// Event alignment for signal_map_batch (nadavca_amd/signal_map.py): per read, an adaptive-banded alignment of its
// events to the k-mer levels of its own bases (Suzuki-Kasahara banding as nanopolish / f5c eventalign use it), the walk
// back and, per base, the first event aligned to it.  The rules are those of include/nadavca_hip.h
// (nvk_event_align_dev); the CPU restatement the tests hold this kernel to is tests/host_shims/eventalign_host.cpp.
//
// One wave64 per read, one block per wave.  The matrix is swept in anti-diagonal bands of BAND = 64 CPL cells; the
// cell at offset o = 64 c + lane of band b is register c of that lane: event i = e0 - o, base j = k0 + o, where
// (e0, k0) is the band's corner.  A band moves right (k0 + 1) or down (e0 + 1) against the one before it, so with r
// the move of this band and r' that of the previous one, the three neighbours of the cell at offset o are
//   stay  (i-1, j)    the previous band's cell at offset o + r
//   skip  (i, j-1)    the previous band's cell at offset o + r - 1
//   step  (i-1, j-1)  the cell of the band before that at offset o + r + r' - 1
// i.e. the two bands kept in registers, moved by at most one offset: a DPP wave rotate by one lane, the lane at the
// seam taking the neighbouring register's end (or -inf at the band's ends).  r and r' are wave-uniform, so which
// rotate runs is a scalar branch.  A move changes either every cell's event or every cell's base; only that half of
// the cell's operands (the level, or mean / ac / mc) is loaded again, a lane keeping the indices it loaded for.  No LDS.
//
// The band's move is decided from the previous band's two end cells (lane 0 of register 0, lane 63 of the last one,
// read into scalars).  Every cell's move (2 bits) goes to the traceback store with two ballots per register: a band is
// 2 CPL 64-bit words, lane k writing word k; the bands' own moves follow as one bit each.  After the sweep the wave
// finds the end cell with a butterfly, walks the path back with wave-uniform loads (lane 0 writes each base's first
// event when the walk leaves the base) and applies the lost rule.  Nothing here depends on which reads share a launch,
// so the host may cut a batch into parts when the store does not fit the workspace cap.
//
// The kernel adds, multiplies and compares doubles and nothing else (no division, log or exp): with
// -ffp-contract=off every score is the rounded operation the contract writes, on the device as on the host.
#include <vector>

#include "kmer_hmm.h"
#include "nvk_internal.h"
#include "part_cut.h"
#include "wave.h"

namespace {

constexpr int EA_MAX = 1 << 26;  // events or bases per read: keeps i + j + 2 and the band count inside int32

struct EventAlignArgs {
  const double *level;       // the events' levels, read j at ev_off[j]
  const int64_t *ev_off;
  const double *mu, *ac, *mc;  // per base, read j at base_off[j]
  const int64_t *base_off;
  const double *l_stay, *l_step;  // per read
  const int32_t *status_in;       // per read or null
  double trim_cost, skip_cost;
  int32_t *out_hit;          // 4 per read: status, events, first event, last event
  double *out_score;
  int32_t *out_base_event;
  unsigned long long *tb;    // the traceback store less the part's first read's tb_off
  const int64_t *tb_off;     // per read, its first word in the batch-wide numbering
  int r0;                    // the part's first read
};

__device__ __forceinline__ double lane_value(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// the band's cells moved by d offsets (-1, 0, 1): out[c] at lane l = the cell at offset 64 c + l + d, -inf outside
template <int CPL>
__device__ __forceinline__ void band_shift(const double (&v)[CPL], int d, int lane, double (&out)[CPL]) {
  const double NINF = nvk_neg_inf();
  if (d == 0) {
#pragma unroll
    for (int c = 0; c < CPL; c++) out[c] = v[c];
  } else if (d > 0) {
    double rot[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) rot[c] = dpp_rol1(v[c]);  // lane l takes lane l + 1, lane 63 lane 0
#pragma unroll
    for (int c = 0; c < CPL; c++) out[c] = lane == 63 ? (c + 1 < CPL ? rot[c + 1 < CPL ? c + 1 : c] : NINF) : rot[c];
  } else {
    double rot[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) rot[c] = dpp_ror1(v[c]);  // lane l takes lane l - 1, lane 0 lane 63
#pragma unroll
    for (int c = 0; c < CPL; c++) out[c] = lane == 0 ? (c > 0 ? rot[c > 0 ? c - 1 : c] : NINF) : rot[c];
  }
}

template <int CPL>
__global__ __launch_bounds__(64) void event_align_kernel(EventAlignArgs a) {
  constexpr int BAND = 64 * CPL, H = BAND / 2, W = 2 * CPL;  // W: traceback words per band
  const double NINF = nvk_neg_inf();
  const int lane = threadIdx.x;
  const int64_t rd = (int64_t)a.r0 + blockIdx.x;
  const int64_t ev0 = a.ev_off[rd], b0 = a.base_off[rd];
  const int E = __builtin_amdgcn_readfirstlane((int)(a.ev_off[rd + 1] - ev0));
  const int K = __builtin_amdgcn_readfirstlane((int)(a.base_off[rd + 1] - b0));
  int status = a.status_in ? __builtin_amdgcn_readfirstlane(a.status_in[rd]) : 0;
  if (status == 0 && (E == 0 || K == 0)) status = NVK_MAP_NO_EVENTS;
  int32_t *be = a.out_base_event + b0;
  if (status != 0) {
    for (int x = lane; x < K; x += 64) be[x] = -1;
    if (lane == 0) {
      *(int4 *)(a.out_hit + 4 * rd) = make_int4(status, E, -1, -1);
      a.out_score[rd] = NINF;
    }
    return;
  }
  const double *lev = a.level + ev0, *mu = a.mu + b0, *ac = a.ac + b0, *mc = a.mc + b0;
  const double l_stay = a.l_stay[rd], l_step = a.l_step[rd], trim = a.trim_cost, skip_cost = a.skip_cost;
  const int nb = E + K + 1;
  unsigned long long *tb = a.tb + a.tb_off[rd];
  unsigned long long *tb_moves = tb + (int64_t)nb * W;

  double p1[CPL], p2[CPL];           // the previous band and the one before it
  double c_lev[CPL], c_mu[CPL], c_ac[CPL], c_mc[CPL];  // the operands of this lane's cells ...
  int at_i[CPL], at_j[CPL];                            // ... and the event and base they were loaded for
#pragma unroll
  for (int c = 0; c < CPL; c++) p1[c] = p2[c] = NINF, c_lev[c] = c_mu[c] = c_ac[c] = c_mc[c] = 0.0, at_i[c] = at_j[c] = -1;
  int e0 = H - 1, k0 = -1 - H;       // the band's corner
  int r_prev = 0;                    // the previous band's move: 1 right, 0 down
  unsigned long long moves = 0;      // the bands' moves, 64 at a time
  double best = NINF;                // this lane's best end cell: largest score, then smallest event
  int best_i = -1;
  for (int b = 0; b < nb; b++) {
    int r = 0;
    if (b >= 2) {
      const double ll = lane_value(p1[0], 0), ur = lane_value(p1[CPL - 1], 63);
      r = (ll == NINF && ur == NINF) ? (b & 1) : (ll < ur ? 1 : 0);
    }
    if (b > 0) {
      e0 += 1 - r;
      k0 += r;
    }
    moves |= (unsigned long long)r << (b & 63);
    double up[CPL], left[CPL], diag[CPL];
    band_shift<CPL>(p1, r, lane, up);
    band_shift<CPL>(p1, r - 1, lane, left);
    band_shift<CPL>(p2, r + r_prev - 1, lane, diag);
    double cur[CPL];
    unsigned mv[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
      const int o = 64 * c + lane;
      const int i = e0 - o, j = k0 + o;
      const bool real = i >= 0 && i < E && j >= 0 && j < K;
      if (real) {
        if (at_i[c] != i) {
          c_lev[c] = lev[i];
          at_i[c] = i;
        }
        if (at_j[c] != j) {
          c_mu[c] = mu[j];
          c_ac[c] = ac[j];
          c_mc[c] = mc[j];
          at_j[c] = j;
        }
      }
      const double em = gauss_log(c_lev[c], c_mu[c], c_ac[c], c_mc[c]);
      const double src = j == 0 ? (double)i * trim : diag[c];
      const double step = (src + l_step) + em;
      const double stay = (up[c] + l_stay) + em;
      const double skip = j > 0 ? left[c] + skip_cost : NINF;
      double v = step;
      unsigned w = 0;
      if (stay > v) {
        v = stay;
        w = 1;
      }
      if (skip > v) {
        v = skip;
        w = 2;
      }
      if (!real) {
        // the trimmed column steers the band and feeds no cell; everything else outside the matrix is -inf
        v = (j == -1 && i >= -1 && i < E) ? (double)(i + 1) * trim : NINF;
        w = 0;
      }
      if (real && j == K - 1) {
        const double end = v + (double)(E - 1 - i) * trim;
        if (end > best || (end == best && best_i >= 0 && i < best_i)) {
          best = end;
          best_i = i;
        }
      }
      cur[c] = v;
      mv[c] = w;
    }
    // the band's moves: word 2 c holds bit 0 of register c's cells, word 2 c + 1 bit 1
    unsigned long long word = 0;
#pragma unroll
    for (int c = 0; c < CPL; c++) {
      const unsigned long long m0 = __ballot(mv[c] & 1u), m1 = __ballot(mv[c] & 2u);
      word = lane == 2 * c ? m0 : lane == 2 * c + 1 ? m1 : word;
    }
    if (lane < W) tb[(int64_t)b * W + lane] = word;
    if (lane == 0 && ((b & 63) == 63 || b == nb - 1)) tb_moves[b >> 6] = moves;
    if ((b & 63) == 63) moves = 0;
#pragma unroll
    for (int c = 0; c < CPL; c++) {
      p2[c] = p1[c];
      p1[c] = cur[c];
    }
    r_prev = r;
  }
  // the end cell over the wave: a cell lies in one band at one offset, so the lanes hold distinct events
  for (int off = 32; off; off >>= 1) {
    const double ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(best_i, off);
    if (oi >= 0 && (best_i < 0 || ov > best || (ov == best && oi < best_i))) {
      best = ov;
      best_i = oi;
    }
  }
  best_i = __builtin_amdgcn_readfirstlane(best_i);
  __syncthreads();  // every lane's traceback stores before the walk reads them
  int first = -1, skipped = 0;
  double score = NINF;
  if (best_i >= 0) {
    // the walk back, by every lane alike (uniform loads); lane 0 stores a base's first event when the walk leaves it.
    // kb: the corner's base of the band the walk stands in, kept by undoing the bands' moves one at a time
    int i = best_i, j = K - 1, fe = -1;
    int bw = nb - 1, kb = k0;
    unsigned long long mword = tb_moves[bw >> 6];
    for (int guard = 0; guard < nb; guard++) {
      const int b = i + j + 2;
      while (bw > b) {
        kb -= (int)((mword >> (bw & 63)) & 1ull);
        bw--;
        if ((bw & 63) == 63) mword = tb_moves[bw >> 6];
      }
      const int o = j - kb;
      // (the moves keep the walk on cells of the bands; the guard keeps every access in bounds regardless)
      if (i < 0 || j < 0 || b < 0 || o < 0 || o >= BAND) break;
      const unsigned long long w0 = tb[(int64_t)b * W + 2 * (o >> 6)], w1 = tb[(int64_t)b * W + 2 * (o >> 6) + 1];
      const unsigned w = (unsigned)((w0 >> (o & 63)) & 1ull) | ((unsigned)((w1 >> (o & 63)) & 1ull) << 1);
      if (w == 2) {
        skipped++;
        if (lane == 0) be[j] = fe;
        fe = -1;
        j--;
        continue;
      }
      fe = i;
      if (w == 1) {
        if (i == 0) break;
        i--;
        continue;
      }
      if (lane == 0) be[j] = fe;
      fe = -1;
      if (j == 0) {
        first = i;
        break;
      }
      i--;
      j--;
    }
  }
  first = __builtin_amdgcn_readfirstlane(first);
  skipped = __builtin_amdgcn_readfirstlane(skipped);
  const bool lost = first < 0 || 8ll * skipped > K;
  if (!lost) score = best;  // (the butterfly left the wave's best in every lane)
  __syncthreads();  // lane 0's stores before the wave overwrites them
  if (lost)
    for (int x = lane; x < K; x += 64) be[x] = -1;
  if (lane == 0) {
    *(int4 *)(a.out_hit + 4 * rd) =
        make_int4(lost ? NVK_MAP_LOST : 0, E, lost ? -1 : first, lost ? -1 : best_i);
    a.out_score[rd] = score;
  }
}

}  // namespace

extern "C" int nvk_event_align_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                                   const int64_t *ev_off, int64_t total_bases, const double *mu, const double *ac,
                                   const double *mc, const int64_t *base_off, const double *l_stay,
                                   const double *l_step, const int32_t *status_in, int band, double trim_cost,
                                   double skip_cost, int32_t *out_hit, double *out_score, int32_t *out_base_event) {
  const char *what = "nvk_event_align_dev";
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff || total_events < 0 || total_bases < 0) {
    nvk_set_error("%s: n_reads %lld, total_events %lld or total_bases %lld out of range", what, (long long)n_reads,
                  (long long)total_events, (long long)total_bases);
    return NVK_ERR_INVALID;
  }
  if (band != 64 && band != 128) {
    nvk_set_error("%s: band %d is not one of the compiled widths 64 and 128", what, band);
    return NVK_ERR_UNSUPPORTED;
  }
  if (int rc = check_log_costs(what, "trim_cost %g or skip_cost %g", {trim_cost, skip_cost})) return rc;
  if (!ev_off || !base_off || (total_events > 0 && !level) || (total_bases > 0 && (!mu || !ac || !mc))) {
    nvk_set_error("%s: NULL levels, offsets or base tables", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> eoff, boff;
  int rc = nvk_fetch_offsets(ctx, "event", ev_off, n_reads, eoff, "total_events", total_events);
  if (rc) return rc;
  if ((rc = nvk_fetch_offsets(ctx, "base", base_off, n_reads, boff, "total_bases", total_bases))) return rc;
  for (int64_t r = 0; r < n_reads; r++)
    if (eoff[r + 1] - eoff[r] > EA_MAX || boff[r + 1] - boff[r] > EA_MAX) {
      nvk_set_error("%s: read %lld has %lld events and %lld bases, above %d", what, (long long)r,
                    (long long)(eoff[r + 1] - eoff[r]), (long long)(boff[r + 1] - boff[r]), EA_MAX);
      return NVK_ERR_INVALID;
    }
  if (n_reads == 0) return NVK_OK;
  if (!l_stay || !l_step || !out_hit || !out_score || (total_bases > 0 && !out_base_event)) {
    nvk_set_error("%s: NULL transition costs or output", what);
    return NVK_ERR_INVALID;
  }
  // the traceback store, in 64-bit words: per read E + K + 1 bands of band / 32 words and one bit per band.  (A read
  // the kernel skips takes its words all the same: its status is on the device.)
  const int64_t W = band / 32;
  std::vector<int64_t> tb_off((size_t)n_reads + 1, 0);
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t nb = (eoff[r + 1] - eoff[r]) + (boff[r + 1] - boff[r]) + 1;
    tb_off[r + 1] = tb_off[r] + nb * W + (nb + 63) / 64;
  }
  // parts of reads whose store fits the cap (a read larger than the cap on its own makes a part of one)
  std::vector<int64_t> cut;
  const int64_t need_w = cut_parts(tb_off, nvk_spill_cap(ctx, WS_SEED_TB) / 8, cut);
  // (the seed aligner's traceback workspaces serve: the two never run at once on a context)
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_TB, (size_t)need_w * 8))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_OFF, ((size_t)n_reads + 1) * sizeof(int64_t) + 64))) return rc;
  int64_t *d_tb_off = (int64_t *)ctx->ws[WS_SEED_OFF];
  NVK_HIP(hipMemcpyAsync(d_tb_off, tb_off.data(), tb_off.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                         ctx->stream));
  EventAlignArgs a;
  a.level = level;
  a.ev_off = ev_off;
  a.mu = mu;
  a.ac = ac;
  a.mc = mc;
  a.base_off = base_off;
  a.l_stay = l_stay;
  a.l_step = l_step;
  a.status_in = status_in;
  a.trim_cost = trim_cost;
  a.skip_cost = skip_cost;
  a.out_hit = out_hit;
  a.out_score = out_score;
  a.out_base_event = out_base_event;
  a.tb_off = d_tb_off;
  for (size_t c = 0; c + 1 < cut.size(); c++) {
    a.r0 = (int)cut[c];
    a.tb = (unsigned long long *)ctx->ws[WS_SEED_TB] - tb_off[cut[c]];
    const dim3 grid((unsigned)(cut[c + 1] - cut[c]));
    if (band == 64)
      hipLaunchKernelGGL(event_align_kernel<1>, grid, dim3(64), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(event_align_kernel<2>, grid, dim3(64), 0, ctx->stream, a);
    NVK_HIP(hipGetLastError());
  }
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
