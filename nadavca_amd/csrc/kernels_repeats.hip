// Repeat counting for count_repeats_batch (nadavca_amd/repeats.py): the Viterbi path of an item's events over a short
// chain of k-mer states with one back edge, the repeat's loop.  The rules are those of include/nadavca_hip.h
// (nvk_repeat_count_dev); the CPU restatement the tests hold this kernel to is tests/host_shims/repeats_host.cpp, which
// keeps the full matrix.
//
// One wave64 per item, one block per wave.  Lane l owns the SPL consecutive states l SPL .. l SPL + SPL - 1 of the
// chain: their mu / ac / mc and the row's cells, all in registers (SPL = 1, 2 or 4 for chains of up to 64, 128 and 256
// states; a state past the chain's end emits -inf and feeds only such states).  A cell is the score S and what a
// traceback would find, carried instead: the times the path went round the loop, its first event, and for each of the
// two marks the candidate value and the event at which the path crossed it.  A row is updated in place from the lane's
// last state down, so the neighbours j - 1 and j - 2 are still the previous row's; at a lane's first states they are the
// previous lane's last two, taken by a DPP wave rotate before the update (lane 0 takes -inf).  The loop's source cell
// is read before the update from the lane that owns it, a wave-uniform lane and slot.  The events are loaded 64 at a
// time, one per lane, and handed out by v_readlane.  The lanes all keep the best end of the chain's last state's slot;
// the lane that owns that state writes the result.  No LDS, no atomics, no workspace.
//
// The kernel adds, multiplies and compares doubles and nothing else: with -ffp-contract=off every score is the rounded
// operation the contract writes, on the device as on the host.
#include <vector>

#include "kmer_hmm.h"
#include "nvk_internal.h"
#include "rep_chain.h"
#include "wave.h"

namespace {

struct RepArgs {
  const int64_t *items;  // per item (chain, ev_lo, ev_hi)
  const double *level;
  const double *mu, *ac, *mc;  // the chains' states, chain c at st_off[c]
  const int64_t *st_off;
  const int32_t *chain_par;  // per chain (lp_from, lp_to, m1, m2)
  const int32_t *status_in;  // per item or null
  double l_stay, l_step, l_skip, trim_cost;
  int32_t *out_hit;
  double *out_score;
};

// what a cell holds: the score, and per mark the candidate value and event of the crossing, the loop count and the
// path's first event
struct RepCell {
  double S, v1, v2;
  int loops, first, i1, i2;
};

__device__ __forceinline__ RepCell rep_unset(double ninf) { return RepCell{ninf, ninf, ninf, 0, -1, -1, -1}; }

__device__ __forceinline__ RepCell rep_ror1(const RepCell &c) {
  return RepCell{dpp_ror1(c.S), dpp_ror1(c.v1), dpp_ror1(c.v2), dpp_ror1(c.loops),
                 dpp_ror1(c.first), dpp_ror1(c.i1), dpp_ror1(c.i2)};
}

// the cell lane `l` holds, l wave-uniform
__device__ __forceinline__ RepCell rep_readlane(const RepCell &c, int l) {
  return RepCell{::rep_readlane(c.S, l),         ::rep_readlane(c.v1, l),         ::rep_readlane(c.v2, l),
                 __builtin_amdgcn_readlane(c.loops, l), __builtin_amdgcn_readlane(c.first, l),
                 __builtin_amdgcn_readlane(c.i1, l),    __builtin_amdgcn_readlane(c.i2, l)};
}

// cell[slot] for a wave-uniform slot, without indexing the registers (field by field: a conditional copy of the whole
// struct becomes a load through a selected pointer, and the row then lives in scratch)
template <int SPL>
__device__ __forceinline__ RepCell rep_slot(const RepCell (&cell)[SPL], int slot) {
  RepCell r = cell[0];
#pragma unroll
  for (int c = 1; c < SPL; c++) {
    const bool s = slot == c;
    r.S = s ? cell[c].S : r.S;
    r.v1 = s ? cell[c].v1 : r.v1;
    r.v2 = s ? cell[c].v2 : r.v2;
    r.loops = s ? cell[c].loops : r.loops;
    r.first = s ? cell[c].first : r.first;
    r.i1 = s ? cell[c].i1 : r.i1;
    r.i2 = s ? cell[c].i2 : r.i2;
  }
  return r;
}

__device__ __forceinline__ void rep_write(const RepArgs &a, int64_t it, int status, int E, int first, int last,
                                          int loops, int i1, int i2, double end, double s_last, double v1, double v2) {
  *(int4 *)(a.out_hit + 8 * it) = make_int4(status, E, first, last);
  *(int4 *)(a.out_hit + 8 * it + 4) = make_int4(loops, i1, i2, 0);
  *(double2 *)(a.out_score + 4 * it) = make_double2(end, s_last);
  *(double2 *)(a.out_score + 4 * it + 2) = make_double2(v1, v2);
}

// SPL states per lane; a wave whose chain another instantiation serves leaves at once
template <int SPL>
__global__ __launch_bounds__(64) void repeat_count_kernel(RepArgs a) {
  const double NINF = nvk_neg_inf();
  const int lane = threadIdx.x;
  const int64_t it = blockIdx.x;
  const int64_t ch = a.items[3 * it];
  const int64_t s0 = a.st_off[ch];
  const int N = __builtin_amdgcn_readfirstlane((int)(a.st_off[ch + 1] - s0));
  if (rep_spl(N) != SPL) return;
  const int64_t e0 = a.items[3 * it + 1];
  const int E = __builtin_amdgcn_readfirstlane((int)(a.items[3 * it + 2] - e0));
  int status = a.status_in ? a.status_in[it] : 0;
  if (status == 0 && E == 0) status = NVK_REP_NO_EVENTS;
  if (status != 0) {
    if (lane == 0) rep_write(a, it, status, E, -1, -1, -1, -1, -1, NINF, NINF, NINF, NINF);
    return;
  }
  const int32_t *par = a.chain_par + 4 * ch;
  const int lp_from = __builtin_amdgcn_readfirstlane(par[0]), lp_to = __builtin_amdgcn_readfirstlane(par[1]);
  const int m1 = __builtin_amdgcn_readfirstlane(par[2]), m2 = __builtin_amdgcn_readfirstlane(par[3]);
  const int from_lane = lp_from / SPL, from_slot = lp_from % SPL, end_slot = (N - 1) % SPL;
  const double *lev = a.level + e0;
  const double l_stay = a.l_stay, l_step = a.l_step, l_skip = a.l_skip, trim = a.trim_cost;

  double mu[SPL], ac[SPL], mc[SPL];
  RepCell cell[SPL];
#pragma unroll
  for (int c = 0; c < SPL; c++) {
    const int j = lane * SPL + c;
    // a state past the chain's end emits -inf: its cells are -inf in every row and feed only such states
    mu[c] = j < N ? a.mu[s0 + j] : 0.0;
    ac[c] = j < N ? a.ac[s0 + j] : NINF;
    mc[c] = j < N ? a.mc[s0 + j] : 0.0;
    cell[c] = rep_unset(NINF);
  }
  double best = NINF;
  int last = -1;
  RepCell at_best = rep_unset(NINF);
  for (int i0 = 0; i0 < E; i0 += 64) {
    const int nb = E - i0 < 64 ? E - i0 : 64;
    const double mine = lane < nb ? lev[i0 + lane] : 0.0;
    for (int t = 0; t < nb; t++) {
      const int i = i0 + t;
      const double e = ::rep_readlane(mine, t);
      const double open = (double)i * trim, tail = (double)(E - 1 - i) * trim;
      // the previous row's loop source, and the previous lane's last two states of the previous row
      const RepCell from = rep_readlane(rep_slot<SPL>(cell, from_slot), from_lane);
      RepCell p1 = rep_ror1(cell[SPL - 1]);
      RepCell p2 = rep_ror1(SPL >= 2 ? cell[SPL >= 2 ? SPL - 2 : 0] : p1);
      if (lane == 0) p1.S = p2.S = NINF;
      if (SPL == 1 && lane == 1) p2.S = NINF;   // (lane 0's p1 before it was cut off)
#pragma unroll
      for (int c = SPL - 1; c >= 0; c--) {
        const int j = lane * SPL + c;
        RepCell s1 = p1, s2 = c == 1 ? p1 : p2;
        if (c >= 1) s1 = cell[c >= 1 ? c - 1 : 0];
        if (c >= 2) s2 = cell[c >= 2 ? c - 2 : 0];
        const double em = gauss_log(e, mu[c], ac[c], mc[c]);
        // v: the largest candidate, the first of equal ones; n: what the cell carries; src: the state it came from
        // (a cell without a finite candidate keeps j and carries nothing)
        double v = NINF;
        RepCell n = rep_unset(NINF);
        int src = j;
        if (j == 0) {
          v = open;
          n.first = i;
          src = -1;
        }
        const double step = s1.S + l_step;
        if (step > v) {
          v = step;
          n = s1;
          src = j - 1;
        }
        const double loop = from.S + l_step;
        if (j == lp_to && loop > v) {
          v = loop;
          n = from;
          n.loops = from.loops + 1;
          src = lp_from;
        }
        const double stay = cell[c].S + l_stay;
        if (stay > v) {
          v = stay;
          n = cell[c];
          src = j;
        }
        const double skip = s2.S + l_skip;
        if (skip > v) {
          v = skip;
          n = s2;
          src = j - 2;
        }
        if (j >= m1 && src < m1) {
          n.v1 = v;
          n.i1 = i;
        }
        if (j >= m2 && src < m2) {
          n.v2 = v;
          n.i2 = i;
        }
        n.S = v + em;
        cell[c] = n;
      }
      // the chain's last state (in the lane that owns it; the other lanes' values are not used)
      const RepCell fin = rep_slot<SPL>(cell, end_slot);
      const double end = fin.S + tail;
      if (end > best) {
        best = end;
        last = i;
        at_best = fin;
      }
    }
  }
  if (lane == (N - 1) / SPL) {
    if (last < 0)
      rep_write(a, it, NVK_REP_NO_PATH, E, -1, -1, -1, -1, -1, NINF, NINF, NINF, NINF);
    else
      rep_write(a, it, NVK_REP_OK, E, at_best.first, last, at_best.loops, at_best.i1, at_best.i2, best, at_best.S,
                at_best.v1, at_best.v2);
  }
}

}  // namespace

extern "C" int nvk_repeat_count_dev(nvk_ctx *ctx, int64_t n_items, const int64_t *items, int64_t total_events,
                                    const double *level, int64_t n_chains, int64_t total_states, const double *mu,
                                    const double *ac, const double *mc, const int64_t *st_off,
                                    const int32_t *chain_par, double l_stay, double l_step, double l_skip,
                                    double trim_cost, const int32_t *status_in, int32_t *out_hit, double *out_score,
                                    double *out_ms) {
  const char *what = "nvk_repeat_count_dev";
  if (out_ms) *out_ms = 0.0;
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_items < 0 || n_items > (1 << 30) || n_chains < 0 || n_chains > 0x7fffffff || total_events < 0 ||
      total_states < 0) {
    nvk_set_error("%s: n_items %lld, n_chains %lld, total_events %lld or total_states %lld out of range", what,
                  (long long)n_items, (long long)n_chains, (long long)total_events, (long long)total_states);
    return NVK_ERR_INVALID;
  }
  if (int rc = check_log_costs(what, "l_stay %g, l_step %g, l_skip %g or trim_cost %g",
                               {l_stay, l_step, l_skip, trim_cost}))
    return rc;
  if (n_items == 0) return NVK_OK;
  if (!items || !st_off || !chain_par || (total_events > 0 && !level) || !mu || !ac || !mc || !out_hit || !out_score) {
    nvk_set_error("%s: NULL items, levels, offsets, chain tables or output", what);
    return NVK_ERR_INVALID;
  }
  bool used[5];   // by states per lane
  if (int rc = rep_check_batch(what, ctx, n_items, items, total_events, n_chains, total_states, st_off, chain_par, used))
    return rc;
  RepArgs a;
  a.items = items;
  a.level = level;
  a.mu = mu;
  a.ac = ac;
  a.mc = mc;
  a.st_off = st_off;
  a.chain_par = chain_par;
  a.status_in = status_in;
  a.l_stay = l_stay;
  a.l_step = l_step;
  a.l_skip = l_skip;
  a.trim_cost = trim_cost;
  a.out_hit = out_hit;
  a.out_score = out_score;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (out_ms) {
    for (hipEvent_t &e : ev) NVK_HIP(hipEventCreate(&e));
    NVK_HIP(hipEventRecord(ev[0], ctx->stream));
  }
  // one wave per item in every instantiation some item's chain needs: the others' waves leave at once
  const dim3 grid((unsigned)n_items);
  if (used[1]) hipLaunchKernelGGL(repeat_count_kernel<1>, grid, dim3(64), 0, ctx->stream, a);
  if (used[2]) hipLaunchKernelGGL(repeat_count_kernel<2>, grid, dim3(64), 0, ctx->stream, a);
  if (used[4]) hipLaunchKernelGGL(repeat_count_kernel<4>, grid, dim3(64), 0, ctx->stream, a);
  NVK_HIP(hipGetLastError());
  if (out_ms) NVK_HIP(hipEventRecord(ev[1], ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  if (out_ms) {
    float ms = 0.f;
    NVK_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *out_ms = (double)ms;
    for (hipEvent_t e : ev) NVK_HIP(hipEventDestroy(e));
  }
  return NVK_OK;
}
