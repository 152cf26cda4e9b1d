// estimate_log_likelihoods on gfx950 (reference: nadavca/dtw/dtw.cpp:37-131; semantics in
// SURVEY.md Appendix A.5, including its two load-bearing quirks).
//
// Per read, one wave64 (persistent, pulls reads from a counter):
//   A. prefix sweep    prefix[0..R]   (dtw.cpp:50-64)
//   B. suffix sweep    suffix[R..0]   (dtw.cpp:66-81) — run as a FORWARD sweep on mirrored
//                      coordinates i' = N - i, so one code path serves both directions
//   C. hypotheses      for every position p and every substituted base b != ref[p]: re-run the
//                      <= k rows the substitution influences, starting from prefix[first] and
//                      closing against suffix[last+1] (dtw.cpp:93-129)
//                      — or, in the LISTED variant (nvk_estimate_hypotheses_batch_dev), only for the (p, b) of the
//                      read's list: the same lanes and arithmetic, the unlisted hypotheses are never run
//                      — or, in the JOINT variant (nvk_estimate_joint_hypotheses_batch_dev), for listed SETS of
//                      substitutions: the rows first = max(0, p1 - back) .. last = min(R - 1, pm + fwd) of the set's
//                      first and last substituted position, every k-mer read with all of them applied, closed at
//                      `last` as a single one is (the items: ell_items.h)
//                      — or, in the EDIT variant (nvk_estimate_edit_hypotheses_batch_dev), for listed insertions /
//                      deletions (p, d, s): the rows around the edit of the EDITED reference, its k-mers, bands and
//                      closing suffix row read through an index map, closed on band last + 1 (the items and the map: ell_items.h)
//
// Mapping (not the reference's): "fused" lanes.  The reference alternates a wobble row
// (mixture of the k-mers j-1 and j, min event length 0) with an emitting row (k-mer j).  Both
// are computed by ONE lane per base position j, which advances two rows per step.  Lanes of
// consecutive positions form a systolic wavefront (cell i of position j at step i + c*j), each
// taking the emitting row from its left neighbour.  All probabilities are scaled linear numbers
// (xmath.h); natural logs are taken once per output value.
//
// Sweep rows are kept row-major in a per-slot row store (16-byte cells: struct Cell) so that phase C reads
// them with unit stride.  Phase C packs 8 hypotheses per wave step in groups of 8 lanes (k-mers longer than 6:
// 4 in groups of 16): a lane for the k-mer before the first position, up to k fused positions, and one closing
// lane that applies the last wobble row and accumulates sum_x cur[x] * suffix[last+1][x].
//
// Wrong-base hypotheses routinely couple quantities that are thousands of bits apart (a k-mer 40 sigma off
// costs ~1000 bits per sample), so every value keeps its own exponent; plain doubles under a shared scale
// were tried and lose exactly the terms that decide such hypotheses.  The scaled numbers are made cheap
// instead:
//   * sums are not re-normalised (xm-style frexp) on every operation: add_lazy aligns the two
//     mantissas and adds, the state is normalised once per trip of 12 steps (phase C: a trip is unrolled, so the
//     history and prefetch slots of a step are constants — fused_step_ring) or every 16 steps (sweeps);
//   * ONE table-based density per lane (dens.h) delivered directly as (mantissa, exponent); the
//     mixture's other component and the predecessor value come from the neighbouring lane with DPP row
//     shifts (lane rho at step u works on the cell lane rho-1 worked on at step u-1) — no LDS traffic;
//   * the three input streams are prefetched in place (no double-buffer copies); cells outside a
//     stream's band are redirected to a zero cell of the row store instead of being masked;
//   * the sweeps use the same arithmetic: a lane's mixture partner is its left neighbour's own density
//     at the same cell, handed over with the emitting value — by a DPP wave rotate at skew 1 (every
//     config-2-shaped read), through an LDS ring otherwise — which is normalised
//     at EVERY hand-over (a dominating value passes its mantissa on; a systematic factor per hand-over
//     would compound to 2^-R or 2^+R along the lanes).
//
// Quirks kept on purpose: the mixture is (g1 + g2) * exp(-2), not / 2; the
// closing wobble row of a hypothesis lives on band row `last`, not `last + 1`.
#include <math.h>
#include <type_traits>

#include "nvk_internal.h"
#include "ell_items.h"
#include "kmer.h"
#include "wave.h"
#include "xmath.h"
#include "dens.h"

namespace {

using xm::X;

constexpr int CH = 128;    // signal refill chunk (samples)
constexpr int TABN = 128;  // descriptor window (two 64-position blocks)
constexpr int PF = 4;      // phase C prefetch depth (steps)
// lanes per hypothesis group (template parameter GL of the kernel): 8 for k-mers up to 6 (8 hypotheses per
// wave step), 16 for longer ones (4 per step; a group is then one DPP row) — phase C needs k + 2 lanes per group
constexpr int HRS = 16;    // sweeps: steps between mantissa normalisations
// exp(-2): the reference divides the mixture by Probability(2) == exp(2) (kmer_model.cpp:59-61)
#define EXPM2_D 0x1.152aaa3bf81ccp-3

// One cell of the row store: 16 bytes, one store / one load (round 3; before: 8 + 4 bytes in two arrays — two
// accesses per cell, and twice as many partly written lines open per wave than the L2 holds: the HBM write traffic
// was 2.7 x the cells).
struct __attribute__((aligned(16))) Cell {
  double m;
  int32_t e;
  int32_t pad;
};
__device__ __forceinline__ void cell_put(Cell *p, X v) {
  *reinterpret_cast<int4 *>(p) = make_int4(__double2loint(v.m), __double2hiint(v.m), v.e, 0);
}
typedef int v3i_t __attribute__((ext_vector_type(3)));
__device__ __forceinline__ X cell_get(const Cell *p) {
  const v3i_t r = *reinterpret_cast<const v3i_t *>(p);  // 12 of the 16 bytes: no register for the padding
  return X{__hiloint2double(r.y, r.x), r.z};
}

struct EllArgs {
  DeviceModel dm;
  BatchArgs a;
  EllPlan pl;
  Cell *store;  // row store: [slot][2][cells]  (prefix rows, then suffix rows)
  int64_t store_stride;  // cells per slot (both halves)
  int64_t half;          // cells per half
  int n_reads;
  int *counter;
  const int *order;  // reads in the order they are handed out (longest first), or null
  int H, SR;
  int c_max;  // largest skew the LDS rings of this launch hold: wider reads get NVK_READ_TOO_WIDE
  int wobbling;
  double *out_ll;
  int32_t *out_status;
};
// A listed variant's arguments: the common ones (out_ll unused), what every listed kind has and the kind's own list, both
// as nvk_internal.h declares them for EllHyp.  items (joint, edit; else null): total_hyp records the read's wave fills
// before its sweeps.  The full variant takes EllArgs alone, so that its kernel arguments stay what they are.
template <class Own>
struct EllHypArgs : EllArgs { EllList list; Own own; int4 *items; };
template <bool LISTED, bool JOINT, bool EDIT>  // (the kernel's three booleans -> its argument)
using EllArgsOf = std::conditional_t<!LISTED, EllArgs, EllHypArgs<std::conditional_t<EDIT, EllEdit,
                                                                  std::conditional_t<JOINT, EllJoint, EllListed>>>>;
using ell_items::JOINT_ROWS;  // the packed items of the joint and the edit variant: ell_items.h

// ---- one fused lane ---------------------------------------------------------------------------
template <int MEL>
struct LaneState {
  X wq[MEL + 1];  // wobble-row values at cells i, i-1, ..., i-MEL
  X em;           // emitting-row value at the previous cell
  X gh[MEL > 0 ? MEL : 1];  // emitting densities of the previous MEL-1.. cells
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k <= MEL; k++) wq[k] = xm::zero();
    em = xm::zero();
#pragma unroll
    for (int k = 0; k < (MEL > 0 ? MEL : 1); k++) gh[k] = xm::one();
  }
};
struct HypDesc {
  double bm, bac, bmc;  // the lane's own density, constants scaled for dens::density
  int wbs, wbe;         // cells of the wobble row (what arrives from the left is taken from wbs on)
  int elo, ebe;         // cells of the emitting row
  int has_wob;
  double wmul;          // phase C: exp(-2) on a lane with a wobble row, 0 without ...
  int wexp;             // ... and 0 / XZ: the mixture times (wmul, wexp) is the mixture or a clean zero
  __device__ __forceinline__ void no_rows() {  // a dead lane: its bands are empty
    wbs = 0x40000000; wbe = -0x40000000; elo = 0x40000000; ebe = -0x40000000;
  }
};

// a + b without re-normalising the mantissa (it drifts by a few bits per step at most; the caller
// normalises every HRS steps).  Zeros carry the exponent XZ, so the other operand passes unchanged.
__device__ __forceinline__ X add_lazy(X a, X b) {
  const int e = max(a.e, b.e);
  return X{ldexp(a.m, a.e - e) + ldexp(b.m, b.e - e), e};
}

// e(x) as (mantissa in [1,2), exponent): dens::density without its final ldexp
// (the polynomial without its g^5 term: 1.2e-15 per density, where the log-likelihoods are compared at 1e-9)
__device__ __forceinline__ X density_x(double x, double mean, double ac, double mc, const double *etab) {
  const double d = x - mean;
  const double y = fma(-(d * d), mc, ac);
  const double kk = rint(y);
  const int ki = (int)kk;
  return X{etab[ki & (dens::ETN - 1)] * dens::dens_poly4(y - kk), ki >> dens::ETL};
}

// One step of a fused lane at cell i, with lazy sums: gb/ga are the two mixture components at the cell's sample,
// pred is the predecessor row at cell i.  Returns the emitting-row value at cell i (`alt` outside its range); the
// wobble value of this cell is left in st.wq[0].
template <int MEL>
__device__ __forceinline__ X fused_step_fast(const HypDesc &d, LaneState<MEL> &st, int i, X gb, X ga,
                                             X pred, X alt) {
  // (g1 + g2) * exp(-2).  Without a wobble row the factor is a clean zero by SELECT: what arrives
  // as `ga` may then be anything (LDS left-overs, the DPP fill value), including NaN, and 0 * NaN
  // would leak it into the row.
  X mix = add_lazy(ga, gb);
  mix.m = (d.has_wob != 0) ? mix.m * EXPM2_D : 0.0;
  mix.e = (d.has_wob != 0) ? mix.e : xm::XZ;
  X wn = add_lazy(pred, xm::mul(mix, st.wq[0]));  // node_next_row.h with mel = 0
  wn = xm::sel(i >= d.wbs && i <= d.wbe, wn, xm::zero());
#pragma unroll
  for (int k = MEL; k >= 1; k--) st.wq[k] = st.wq[k - 1];
  st.wq[0] = wn;
  X P = xm::one();
  if (MEL >= 1) {
    P = gb;
#pragma unroll
    for (int k = 0; k < MEL - 1; k++) P = xm::mul(P, st.gh[k]);
  }
  X en = add_lazy(xm::mul(P, st.wq[MEL]), xm::mul(gb, st.em));
  en = xm::sel(i >= d.elo && i <= d.ebe, en, alt);  // alt: a zero (the sweeps), the lane's stream (phase C)
  st.em = en;
  if (MEL >= 2) {
#pragma unroll
    for (int k = MEL - 2; k >= 1; k--) st.gh[k] = st.gh[k - 1];
    st.gh[0] = gb;
  }
  return en;
}

// fused_step_fast with the wobble history as a ring: the value of step u lives in wq[u % (MEL+1)] (r, a constant
// once the caller's trip of lcm(PF, MEL+1) steps is unrolled), so no register moves between steps
template <int MEL>
__device__ __forceinline__ void fused_step_ring(const HypDesc &d, LaneState<MEL> &st, int r, int i, X gb, X ga,
                                                X pred, X alt) {
  constexpr int M = MEL + 1;
  // (g1 + g2) * exp(-2), or a zero without a wobble row — by multiplication: both densities are finite here (a
  // lane's own, and its left neighbour's through the DPP move, whose fill value is 0), so 0 * mix is 0
  X mix = add_lazy(ga, gb);
  mix.m = mix.m * d.wmul;
  mix.e = mix.e + d.wexp;
  X wn = add_lazy(pred, xm::mul(mix, st.wq[(r + M - 1) % M]));
  // Outside its band the wobble value only gets the exponent of a zero (one select instead of three): beside any
  // real number such a value vanishes exactly (ldexp by -2^28 is 0), beside another of its kind it stays one, and a
  // total made of nothing else is recognised by its exponent when the hypothesis is finished (below XZ / 2: a zero).
  wn.e = (i >= d.wbs && i <= d.wbe) ? wn.e : xm::XZ;
  st.wq[r] = wn;  // replaces the value of step u - M; the one of step u - MEL is wq[(r + 1) % M]
  X en;
  if (MEL >= 1) {
    // e(s_i) * (e(s_{i-1}) .. e(s_{i-MEL+1}) * wobble[i-MEL] + emitting[i-1]): the newest density taken out of both
    // terms (two multiplications fewer than product-first; the rounding differs in the last bit)
    X Q = st.wq[(r + 1) % M];
#pragma unroll
    for (int k = 0; k < MEL - 1; k++) Q = xm::mul(Q, st.gh[k]);
    en = xm::mul(gb, add_lazy(Q, st.em));
  } else {
    en = add_lazy(st.wq[(r + 1) % M], xm::mul(gb, st.em));
  }
  // alt: the lane's stream at this cell (see the caller).  Only the row's LAST cell is tested: below its first
  // one the wobble history and the previous value are (such) zeros already.
  en = xm::sel(i <= d.ebe, en, alt);
  st.em = en;
  if (MEL >= 2) {
#pragma unroll
    for (int k = MEL - 2; k >= 1; k--) st.gh[k] = st.gh[k - 1];
    st.gh[0] = gb;
  }
}

// the DPP moves of wave.h for a scaled number.  dpp_shr1: the first lane of each 16-lane row reads 0 — those lanes
// are role 0 of a group and never use what arrives from the left; dpp_ror1: the sweeps' hand-over at skew 1
__device__ __forceinline__ X dpp_shr1(X v) {
  return X{::dpp_shr1(v.m), __builtin_amdgcn_mov_dpp(v.e, 0x111, 0xf, 0xf, true)};
}
__device__ __forceinline__ X dpp_ror1(X v) { return X{::dpp_ror1(v.m), ::dpp_ror1(v.e)}; }

// One sweep over the R fused positions of `desc` (prefix order or mirrored suffix order), with the arithmetic of
// the hypothesis phase: lazy sums, one table density per lane; the mixture's other component is the left
// neighbour's own density at the same cell, which the neighbour evaluated c steps earlier and hands over through
// the LDS ring together with its emitting value (24 B per lane and slot).
// a FusedParam as a sweep lane holds it in the LDS window: the constants scaled
struct __attribute__((aligned(16))) SweepLane {
  double bm, bac, bmc;  // the emitting Gaussian, constants scaled for dens::density
  int32_t wbs, wbe, ebe, ebs, soff, has_wob;
};
static_assert(sizeof(SweepLane) == 48, "SweepLane layout");

__device__ __forceinline__ void load_lane_block(SweepLane *tab, const FusedParam *src, int blk, int R,
                                                int lane) {
  int j = blk * 64 + lane;
  if (j >= 0 && j < R) {
    const FusedParam f = src[j];
    SweepLane l;
    l.bm = f.b_mean;
    dens::scale_consts(f.b_ac, f.b_mc, l.bac, l.bmc);
    l.wbs = f.wbs; l.wbe = f.wbe; l.ebe = f.ebe; l.ebs = f.ebs; l.soff = f.store_off;
    l.has_wob = f.has_wob;
    tab[j & (TABN - 1)] = l;
  }
}

// SK1: the read's skew is 1 (every config-2-shaped read: a lane is done with its row before the row 64 further
// on begins) — the left neighbour's values of ONE step ago are one DPP wave rotate away, and the history rings in
// LDS, their six accesses per step and the wave barrier between a step's write and the next step's read are not
// needed.  Other skews keep the rings.
template <int MEL, bool SK1>
__device__ void sweep_fast(const FusedParam *desc, int R, int N, int c, const double *sig, bool mirror,
                           double *ring, int RM, SweepLane *tab, const double *etab, double *hist_m,
                           double *hist_g, int *hist_e, int H, Cell *rows_out, int lane) {
  int r_old = 0, loaded_hi = 0;
  load_lane_block(tab, desc, 0, R, lane);
  __syncthreads();
  int j = lane;
  HypDesc d;
  int ebs = 0, soff = 0;
  auto take = [&](const SweepLane &f) {
    d.bm = f.bm; d.bac = f.bac; d.bmc = f.bmc;
    d.has_wob = f.has_wob;
    d.wbs = f.wbs; d.wbe = f.wbe; d.ebe = f.ebe;
    d.elo = max(f.wbs, MEL);
    ebs = f.ebs; soff = f.soff;
  };
  d.bm = d.bac = d.bmc = 0.0; d.has_wob = 0;
  d.no_rows();
  if (j < R) take(tab[j & (TABN - 1)]);
  const int t_min = __builtin_amdgcn_readfirstlane(d.wbs);
  const FusedParam &lastf = desc[R - 1];
  const int t_max = lastf.ebe + c * (R - 1);
  const int n_steps = __builtin_amdgcn_readfirstlane(t_max - t_min + 1);
  LaneState<MEL> st;
  st.reset();
  int i = t_min - c * j;
  int filled_hi = ((t_min - 1) > 0 ? (t_min - 1) / CH : 0) * CH;
  auto fill = [&](int upto) {
    while (upto >= filled_hi) {
      __syncthreads();
      for (int w = lane; w < CH; w += 64) {
        int idx = filled_hi + w;
        int src = mirror ? (N - 1 - idx) : idx;
        ring[idx & RM] = (idx >= 0 && idx < N) ? sig[src] : 0.0;
      }
      filled_hi += CH;
      __syncthreads();
    }
  };
  fill(t_min);
  int su = 0, sr = ((-c) % H + H) % H;
  X pe = xm::zero(), pg = xm::one();  // SK1: this lane's emitting value and density of the previous step
  for (int u = 0; u < n_steps; ++u) {
    const int t = t_min + u;
    bool fin = (i > d.ebe) && (j < R);
    if (__any(fin)) {
      int nj = j + 64;
      if (__any(fin && nj < R && (nj >> 6) > loaded_hi)) {
        loaded_hi++;
        load_lane_block(tab, desc, loaded_hi, R, lane);
        __syncthreads();
      }
      if (fin) {
        j = nj;
        i -= 64 * c;
        st.reset();
        if (j < R) take(tab[j & (TABN - 1)]);
        else d.no_rows();
      }
      while (r_old < R && __builtin_amdgcn_readlane(j, r_old & 63) != r_old) r_old++;
    }
    if (r_old < R) fill(t - c * r_old);
    if ((u & (HRS - 1)) == HRS - 1) {  // keep the lazily summed mantissas of the wobble row near 1
      asm volatile("");
#pragma unroll
      for (int k = 0; k <= MEL; k++) st.wq[k] = xm::norm(st.wq[k]);
    }
    const double x = ring[(i - 1) & RM];
    // left neighbour, c steps ago, same cell: its emitting value (zero beyond its last cell; only
    // taken from the wobble row's first cell on) and its density
    X pred, ga;
    if (SK1) {
      pred = dpp_ror1(pe);
      ga = dpp_ror1(pg);
    } else {
      const int hs = sr * 64 + ((lane - 1) & 63);
      pred = X{hist_m[hs], hist_e[2 * hs]};
      ga = X{hist_g[hs], hist_e[2 * hs + 1]};
    }
    if (j == 0) pred = xm::one();  // prefix[0] / suffix[R]: all ones on their band
    const X gb = density_x(x, d.bm, d.bac, d.bmc, etab);
    // The emitting value is handed from lane to lane R times: it is normalised on EVERY step.  A value
    // that dominates the sums it enters passes its mantissa on, so any systematic factor per hand-over
    // (the 0.5 of xm::one() with mel = 0, the emission product's mantissa otherwise) would compound to
    // 2^-R or 2^+R along the lanes, whatever the lanes do to their own registers in between.
    (void)fused_step_fast<MEL>(d, st, i, gb, ga, pred, xm::zero());
    st.em = xm::norm(st.em);
    const X en = st.em;
    if (SK1) {
      pe = en;
      pg = gb;
    } else {
      const int hw = su * 64 + lane;
      hist_m[hw] = en.m;
      hist_g[hw] = gb.m;
      *reinterpret_cast<int2 *>(hist_e + 2 * hw) = make_int2(en.e, gb.e);
    }
    if (i >= ebs && i <= d.ebe) {  // row-major store, un-mirrored cell index
      int off = soff + (mirror ? (d.ebe - i) : (i - ebs));
      cell_put(rows_out + off, en);
    }
    i += 1;
    if (!SK1) {
      su = (su + 1 == H) ? 0 : su + 1;
      sr = (sr + 1 == H) ? 0 : sr + 1;
      WAVE_SYNC();
    }
  }
}

template <int MEL, int GL, bool LISTED, bool JOINT = false, bool EDIT = false>
__global__ __launch_bounds__(64, 3) void ell_kernel(EllArgsOf<LISTED, JOINT, EDIT> g) {
  static_assert(LISTED || !JOINT, "the joint variant is a listed one");
  static_assert(JOINT || !EDIT, "the edit variant takes its work from items, as the joint one");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *etab = reinterpret_cast<double *>(smem);
  double *ring = etab + dens::ETN;
  SweepLane *tab = reinterpret_cast<SweepLane *>(ring + g.SR);
  double *hist_m = reinterpret_cast<double *>(tab + TABN);
  double *hist_g = hist_m + (size_t)g.H * 64;  // the lanes' own densities
  int *hist_e = reinterpret_cast<int *>(hist_g + (size_t)g.H * 64);
  int *s_read = hist_e + (size_t)g.H * 64 * 2;

  const int lane = threadIdx.x;
  const int RM = g.SR - 1;
  const DeviceModel dm = g.dm;
  const int alpha = dm.alphabet;
  Cell *pre = g.store + (size_t)blockIdx.x * g.store_stride;
  Cell *suf = pre + g.half;
  for (int q = lane; q < g.SR; q += 64) ring[q] = 0.0;
  dens::fill_table(etab, lane, 64);
  if (lane == 0) {  // the store's last cell is never part of a row: a zero the streams can point at
    cell_put(pre + g.store_stride - 1, xm::zero());
  }

  while (true) {
    __syncthreads();
    if (lane == 0) *s_read = atomicAdd(g.counter, 1);
    __syncthreads();
    const int pos = __builtin_amdgcn_readfirstlane(*s_read);
    if (pos >= g.n_reads) break;
    const int rd = g.order ? g.order[pos] : pos;
    const ReadMeta m = g.pl.metas[rd];
    const int R = __builtin_amdgcn_readfirstlane(m.R);
    double *out = LISTED ? nullptr : g.out_ll + (size_t)m.ref_off * alpha;
    if (m.status != NVK_READ_OK) {
      if (lane == 0) g.out_status[rd] = m.status;
      continue;
    }
    // LISTED: the read's hypotheses; one outside the read or the alphabet fails the read before any table is indexed
    int64_t h0 = 0;
    int n_list = 0;
    int n_small = 0;  // JOINT: the items that fit a group of GL lanes come first in g.items, the others after them
    if constexpr (JOINT) {
      // one lane per hypothesis: check its substitutions, pack the effective ones (b != ref[p]) and file the item
      // under the lanes it needs — those of at most GL - 2 rows from the front, the others from the back
      h0 = g.list.off[rd];
      n_list = __builtin_amdgcn_readfirstlane((int)(g.list.off[rd + 1] - h0));
      const int back_ = dm.k - dm.central - 1, fwd_ = dm.central;
      int n_big = 0;
      bool bad = false;
      for (int q0 = 0; q0 < n_list; q0 += 64) {
        const int q = q0 + lane;
        const bool have = q < n_list;
        int p1 = 0, rows = 1;
        ell_items::code_t code = 0;
        if constexpr (EDIT) {
          if (have && !bad) {
            // (host-checked offsets: the letter count is >= 0, and the letters read lie inside ins_base)
            const int64_t s0 = g.own.ins_off[h0 + q];
            p1 = g.own.pos[h0 + q];
            bad = !ell_items::edit_pack(R, alpha, back_, fwd_, p1, g.own.del[h0 + q], g.own.ins_base + s0,
                                        g.own.ins_off[h0 + q + 1] - s0, code, rows);
          }
        } else if (have) {
          const int64_t s0 = g.own.sub_off[h0 + q];
          bad = !ell_items::joint_pack(g.a.reference + m.ref_off, R, alpha, back_, fwd_, g.own.sub_pos + s0, g.own.sub_base + s0,
                                       g.own.sub_off[h0 + q + 1] - s0, p1, code, rows) || bad;
        }
        const bool small = GL == 16 || rows + 2 <= GL;
        const unsigned long long ms = __ballot(have && small), mb = __ballot(have && !small);
        const unsigned long long below = (1ull << lane) - 1;
        const int slot = small ? n_small + __popcll(ms & below) : n_list - 1 - n_big - __popcll(mb & below);
        if (have) g.items[h0 + slot] = make_int4(p1, q, ell_items::code_lo(code), ell_items::code_hi(code));
        n_small += __popcll(ms);
        n_big += __popcll(mb);
      }
      if (__any(bad)) {
        if (lane == 0) g.out_status[rd] = NVK_READ_BAD_INPUT;
        continue;
      }
    } else if constexpr (LISTED) {
      h0 = g.list.off[rd];
      n_list = __builtin_amdgcn_readfirstlane((int)(g.list.off[rd + 1] - h0));
      bool bad = false;
      for (int q = lane; q < n_list; q += 64) {
        const int hp = g.own.pos[h0 + q], hb = g.own.base[h0 + q];
        bad = bad || hp < 0 || hp >= R || hb < 0 || hb >= alpha;
      }
      if (__any(bad)) {
        if (lane == 0) g.out_status[rd] = NVK_READ_BAD_INPUT;
        continue;
      }
    }
    const int N = __builtin_amdgcn_readfirstlane(m.N);
    const int c = __builtin_amdgcn_readfirstlane(m.c);
    if (c > g.c_max) {  // the band does not fit one wave's rings: this read only
      if (lane == 0) g.out_status[rd] = NVK_READ_TOO_WIDE;
      continue;
    }
    const double *sig = g.a.signal + m.sig_off;
    const char *sig_u;  // the same address as a scalar (phase C loads with scalar base + 32-bit lane offset)
    {
      const unsigned long long a = (unsigned long long)sig;
      sig_u = (const char *)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                             (unsigned)__builtin_amdgcn_readfirstlane((int)a));
    }
    const int32_t *ref = g.a.reference + m.ref_off;
    const int nb = (int)(g.a.cb_off[rd + 1] - g.a.cb_off[rd]);
    const int na = (int)(g.a.ca_off[rd + 1] - g.a.ca_off[rd]);
    const int32_t *cb = g.a.ctx_before + g.a.cb_off[rd];
    const int32_t *ca = g.a.ctx_after + g.a.ca_off[rd];
    const int32_t *bs = g.pl.bs + m.ref_off + rd;
    const int32_t *be = g.pl.be + m.ref_off + rd;
    const int32_t *rowoff = g.pl.rowoff + m.ref_off + rd;

    // rows that are all ones: prefix[0] on band 0, suffix[R] on band R (dtw.cpp:50,66-67)
    for (int x = bs[0] + lane; x <= be[0]; x += 64) {
      cell_put(pre + rowoff[0] + x - bs[0], xm::one());
    }
    for (int x = bs[R] + lane; x <= be[R]; x += 64) {
      cell_put(suf + rowoff[R] + x - bs[R], xm::one());
    }
    // ---- A, B: the two sweeps
    if (c == 1) {
      sweep_fast<MEL, true>(g.pl.fwd + m.row_off, R, N, c, sig, false, ring, RM, tab, etab, hist_m, hist_g, hist_e,
                            g.H, pre, lane);
      __syncthreads();
      sweep_fast<MEL, true>(g.pl.rev + m.row_off, R, N, c, sig, true, ring, RM, tab, etab, hist_m, hist_g, hist_e,
                            g.H, suf, lane);
    } else {
      sweep_fast<MEL, false>(g.pl.fwd + m.row_off, R, N, c, sig, false, ring, RM, tab, etab, hist_m, hist_g, hist_e,
                             g.H, pre, lane);
      __syncthreads();
      sweep_fast<MEL, false>(g.pl.rev + m.row_off, R, N, c, sig, true, ring, RM, tab, etab, hist_m, hist_g, hist_e,
                             g.H, suf, lane);
    }
    __syncthreads();

    // ---- no-substitution likelihood: sum_x prefix[R][x] * suffix[R][x]  (dtw.cpp:83-85)
    X tot = xm::zero();
    for (int x = bs[R] + lane; x <= be[R]; x += 64) {
      int o = rowoff[R] + x - bs[R];
      X v = xm::mul(cell_get(pre + o), cell_get(suf + o));
      tot = xm::add_norm(tot, v);
    }
    for (int dlt = 32; dlt >= 1; dlt >>= 1) {
      X o{__shfl_xor(tot.m, dlt, 64), __shfl_xor(tot.e, dlt, 64)};
      tot = xm::add_norm(tot, o);
    }
    const double no_snp = xm::to_log(tot);
    if constexpr (LISTED) {
      if (lane == 0) g.list.out_total[rd] = no_snp;
    } else {
      for (int p = lane; p < R; p += 64) out[(size_t)p * alpha + ref[p]] = no_snp;
    }

    // ---- C: substitution hypotheses, 8 per wave step
    const int back = dm.k - dm.central - 1, fwd = dm.central;
    const int n_items = LISTED ? n_list : R * (alpha - 1);
    // lane roles in a group: 0 = density of the k-mer before `first` (only feeds the mixture of the
    // first position), 1..npos = the positions first..last, npos+1 = the closing lane.
    // Lane role rho is at cell i = base + u - rho at step u, so whatever lane rho-1 produced at step
    // u-1 (emitting value, density) belongs to the cell lane rho works on at step u.
    const int smax = 2 * (int)g.half - 1;
    if constexpr (JOINT) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // g.items: other lanes wrote them
    // JOINT with groups of 8 lanes: the items [0, n_small) 8 per wave step as in the listed variant, then the others
    // in groups of 16 lanes, 4 per step — one loop, the group width a uniform of the step.  No step mixes widths:
    // a narrow step advances b0 by 64 / GL items but never past n_small, so b0 lands on n_small exactly, the last
    // narrow step serves only the items below it (`valid`), and every step from there on is wide
    constexpr bool TWO_WIDTHS = JOINT && GL < 16;
    const int grp_gl = lane / GL, gl_gl = lane % GL;
    for (int b0 = 0; b0 < n_items;) {
      const bool wide = TWO_WIDTHS && b0 >= n_small;
      const int grp = wide ? lane / 16 : grp_gl, gl = wide ? lane % 16 : gl_gl;
      const int item = b0 + grp;
      const bool valid = item < (TWO_WIDTHS && !wide ? n_small : n_items);
      if constexpr (TWO_WIDTHS) b0 = wide ? b0 + 4 : min(b0 + 64 / GL, n_small);
      else b0 += 64 / GL;
      int p = 0, b = 0, first = 0, last = 0, npos = 0;
      [[maybe_unused]] int hidx = 0;
      [[maybe_unused]] ell_items::code_t code = 0;
      [[maybe_unused]] ell_items::Edit ed = {0, 0, 0, 0};
      if constexpr (JOINT) {
        if (valid) {
          const int4 it = g.items[h0 + item];
          p = it.x;
          hidx = it.y;
          code = ell_items::code_of(it.z, it.w);
          if constexpr (EDIT) {
            ed = ell_items::edit_unpack(p, code);
            first = ell_items::edit_first(ed, back);
            last = ell_items::edit_last(ed, R, fwd);
          } else {
            first = ell_items::joint_first(p, back);
            last = ell_items::joint_last(R, p + ell_items::joint_span(code), fwd);
          }
          npos = last - first + 1;
        }
      } else if (valid) {
        if constexpr (LISTED) {
          p = g.own.pos[h0 + item];
          b = g.own.base[h0 + item];
        } else {
          p = item / (alpha - 1);
          int bi = item % (alpha - 1);
          b = bi + (bi >= ref[p] ? 1 : 0);
        }
        first = max(0, p - back);
        last = min(R - 1, p + fwd);
        npos = last - first + 1;
      }
      // k-mer id of position `at` under the hypothesis: base p replaced by b, or (joint) the bases the item
      // substitutes, or (edit) position `at` of the edited reference, through the edit map
      auto kid = [&](int at) {
        if constexpr (EDIT)
          return kmer_id_mapped(dm, ref, R, cb, nb, ca, na, at,
                                [&](int &j, int &v) { return ell_items::edit_at(ed, j, v); });
        else if constexpr (JOINT)
          return kmer_id(dm, ref, R, cb, nb, ca, na, at,
                         [&](int j, int &v) { return ell_items::joint_at(p, code, j, v); });
        else
          return kmer_id(dm, ref, R, cb, nb, ca, na, at, [&](int j, int &v) { v = b; return j == p; });
      };
      // boundary row r of the hypothesis' reference as a row of the read's band arrays (bs / be): itself, except EDIT
      auto row_s = [&](int r) {
        if constexpr (EDIT) return ell_items::edit_row_s(ed, r);
        else return r;
      };
      auto row_e = [&](int r) {
        if constexpr (EDIT) return ell_items::edit_row_e(ed, r);
        else return r;
      };
      const bool is_pos = valid && gl >= 1 && gl <= npos;
      const bool is_fin = valid && gl == npos + 1;
      HypDesc d;
      d.no_rows();
      d.has_wob = 0; d.bm = 0.0; d.bac = 0.0; d.bmc = 0.0;
      // input stream of the lane: cell i lives at pre[sbase + i] (the suffix rows follow the
      // prefix rows in the same store, g.half cells on), valid for i in [slo, shi]; every other cell
      // reads the store's zero cell
      int sbase = 0, slo = 0x40000000, shi = -0x40000000;
      int64_t idb = -1;
      if (valid && gl == 0) {
        if (first > 0 && g.wobbling) idb = kid(first - 1);
        // this lane also carries prefix[first] to the first position: its rows are empty, so what it keeps as
        // "emitting value" is the alternative of the band select — its stream at the cell it is on, which is
        // the cell the lane to its right works on one step later
        sbase = rowoff[first] - bs[first];
        slo = bs[first]; shi = be[first];
      } else if (is_pos) {
        const int j = first + gl - 1;
        idb = kid(j);
        d.has_wob = (j > 0 && g.wobbling) ? 1 : 0;
        d.wbs = bs[row_s(j)]; d.wbe = be[row_e(j)]; d.ebe = be[row_e(j + 1)];
      } else if (is_fin && EDIT) {
        // closing lane of an edit: no quirk — the wobble row lives on band last + 1, where the prefix sweep puts it
        // (dtw.cpp:53-58), so the value is the total of the edited reference.  Boundary row last + 1 lies behind the
        // edit: it is the read's row `close`, whose band it has and whose suffix row closes the hypothesis
        const int close = ell_items::edit_close(ed, last);
        d.has_wob = (close < R && g.wobbling) ? 1 : 0;
        if (d.has_wob) idb = kid(last + 1);
        d.wbs = bs[close]; d.wbe = be[close];
        d.ebe = d.wbe;
        sbase = (int)g.half + rowoff[close] - bs[close];
        slo = bs[close]; shi = be[close];
      } else if (is_fin) {
        // closing lane: optional wobble row on band `last` (quirk), predecessor = emitting row of
        // position `last` on band last+1; then the running total against suffix[last+1]
        d.has_wob = (last + 1 < R && g.wobbling) ? 1 : 0;
        if (d.has_wob) {
          idb = kid(last + 1);
          // band `last`; the emitting row of `last` only exists from bs[last+1] on, and nothing
          // can be in the wobble row before its first value arrives
          d.wbs = max(bs[last], bs[last + 1]); d.wbe = be[last];
        } else {
          d.wbs = bs[last + 1]; d.wbe = be[last + 1];
        }
        d.ebe = d.wbe;
        sbase = (int)g.half + rowoff[last + 1] - bs[last + 1];
        slo = bs[last + 1]; shi = be[last + 1];
      }
      if (idb >= 0) {
        d.bm = dm.mean[idb];
        dens::scale_consts(dm.ac[idb], dm.mc[idb], d.bac, d.bmc);
      }
      d.elo = max(d.wbs, MEL);
      d.wmul = d.has_wob ? EXPM2_D : 0.0;
      d.wexp = d.has_wob ? 0 : xm::XZ;
      const int base = valid ? bs[first] : 0;
      int steps = 0;
      if (is_fin) steps = d.wbe - base + gl + 1;
      steps = __builtin_amdgcn_readfirstlane(wave_max(steps));  // uniform trip count
      const int i0 = base - gl;
      // clamped, unsigned element offsets from uniform base pointers (scalar base + 32-bit offset)
      // byte offset of the stream's cell i from the slot's (scalar) base; the store's zero cell outside the band
      const int sb16 = 16 * sbase;
      auto sload = [&](int i) {
        const unsigned off = (unsigned)((i >= slo && i <= shi) ? sb16 + 16 * i : 16 * smax);
        return cell_get(reinterpret_cast<const Cell *>(reinterpret_cast<const char *>(pre) + off));
      };
      // sample s[i-1] of cell i, clamped into the read (cells beyond it are outside every band): a byte offset
      // from the read's uniform base pointer, one v_med3 per load
      const int xhi = 8 * (N - 1);
      auto xload = [&](int i) {
        int off;
        asm("v_med3_i32 %0, %1, 0, %2" : "=v"(off) : "v"(8 * (i - 1)), "s"(xhi));
        return *reinterpret_cast<const double *>(sig_u + (unsigned)off);
      };
      LaneState<MEL> st;
      st.reset();
      X acc = xm::zero(), gb_last = xm::one();
      double cx[PF];
      X cs[PF];
#pragma unroll
      for (int q = 0; q < PF; q++) {
        cx[q] = xload(i0 + q);
        cs[q] = sload(i0 + q);
      }
      // a trip = lcm(PF, MEL + 1) steps, unrolled: prefetch slot and history slot of every step are constants.
      // The steps are rounded up to whole trips (the extra cells lie beyond every band: zeros, zero cell).
      // (min event length 4: 20 steps per trip are more than the register allocator survives; that variant
      // keeps PF steps per trip and shifts its history)
      constexpr int M = MEL + 1;
      constexpr bool RING = (PF % M == 0) || PF * M <= 12;
      constexpr int TRIP = (!RING || PF % M == 0) ? PF : PF * M;
      constexpr int NRM = (11 / TRIP + 1) * TRIP;  // steps between mantissa normalisations: whole trips, >= 12
      for (int ub = 0; ub < steps; ub += TRIP) {
#pragma unroll
        for (int w = 0; w < TRIP; w++) {
          const int q = w % PF, r = w % M;
          const int u = ub + w;
          const int i = i0 + u;
          const X sv = cs[q];  // zero outside the stream's band (zero cell)
          const X ga = dpp_shr1(gb_last);
          // the emitting row of the lane to the left, one step ago: zero beyond its last cell, and only taken
          // from the wobble row's first cell on; for the first position that lane is role 0, which hands
          // prefix[first] over.  Outside its emitting row a lane keeps `sv` instead of a zero: the zero cell for
          // every position lane (they have no stream), the stream for role 0, and nobody reads the closing lane's
          const X pred = dpp_shr1(st.em);
          const X gb = density_x(cx[q], d.bm, d.bac, d.bmc, etab);
          if constexpr (RING)
            fused_step_ring<MEL>(d, st, r, i, gb, ga, pred, sv);
          else
            (void)fused_step_fast<MEL>(d, st, i, gb, ga, pred, sv);
          gb_last = gb;
          // node.cpp:31-37; only the closing lane's total is used (the other lanes sum garbage)
          acc = add_lazy(acc, xm::mul(st.wq[RING ? r : 0], sv));
          cx[q] = xload(i0 + u + PF);
          cs[q] = sload(i0 + u + PF);
        }
        if ((ub + TRIP) % NRM == 0) {  // keep the lazily summed mantissas near 1
#pragma unroll
          for (int k = 0; k <= MEL; k++) st.wq[k] = xm::norm(st.wq[k]);
          st.em = xm::norm(st.em);
          acc = xm::norm(acc);
        }
      }
      if (is_fin) {
        acc = xm::norm(acc);
        if (RING && acc.e < xm::XZ / 2) acc = xm::zero();  // made of nothing but out-of-band values (fused_step_ring)
        // LISTED: b == ref[p] is no substitution — the total of the two sweeps, as the full matrix holds it there
        if constexpr (JOINT) g.list.out_hyp[h0 + hidx] = code == 0 ? no_snp : xm::to_log(acc);
        else if constexpr (LISTED) g.list.out_hyp[h0 + item] = (b == ref[p]) ? no_snp : xm::to_log(acc);
        else out[(size_t)p * alpha + b] = xm::to_log(acc);
      }
    }
    // a read without any valid path has likelihood zero everywhere (the reference returns an
    // all -inf matrix, which its estimator then turns into NaN): report it per read instead
    if (lane == 0) g.out_status[rd] = (no_snp == -INFINITY) ? NVK_READ_NO_PATH : NVK_READ_OK;
  }
}

}  // namespace

namespace {
// One variant's launch: its argument struct from the common part `base` and the variant's lists in `hyp`, the
// instantiation for the batch's min event length and group width, `slots` blocks of one wave with `lds` bytes.
template <bool LISTED, bool JOINT, bool EDIT>
int ell_dispatch(nvk_ctx *ctx, const EllArgs &base, const EllHyp &hyp, bool wide_groups, int64_t slots, size_t lds) {
  typedef EllArgsOf<LISTED, JOINT, EDIT> Args;
  Args g;
  static_cast<EllArgs &>(g) = base;
  if constexpr (LISTED) g.list = hyp.list;
  if constexpr (EDIT) g.own = hyp.edit;
  else if constexpr (JOINT) g.own = hyp.joint;
  else if constexpr (LISTED) g.own = hyp.listed;
  if constexpr (LISTED) g.items = JOINT ? (int4 *)ctx->ws[WS_JOINT] : nullptr;
  // What is built: M of 0..4 (the batch's min event length, checked by launch_ell) x {8, 16} lanes per hypothesis (the
  // table's k: k + 2 <= 8 or not) x the four kinds (the entry point), 5 x 2 x 4 = 40 kernels, all of them reachable.
#define ELL_PAIR(M) {ell_kernel<M, 8, LISTED, JOINT, EDIT>, ell_kernel<M, 16, LISTED, JOINT, EDIT>}
  static void (*const kernels[5][2])(Args) = {ELL_PAIR(0), ELL_PAIR(1), ELL_PAIR(2), ELL_PAIR(3), ELL_PAIR(4)};
#undef ELL_PAIR
  void (*const kern)(Args) = kernels[base.a.mel][wide_groups ? 1 : 0];
  if (lds > 64 * 1024) {
    NVK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  {
    TimerScope ts(ctx, NVK_K_ELL_HYP);
    hipLaunchKernelGGL(kern, dim3((unsigned)slots), dim3(64), lds, ctx->stream, g);
  }
  NVK_HIP(hipGetLastError());
  // launch report (include/nadavca_hip.h)
  nvk_launch_note(ctx, nvk_launch_rec{NVK_LAUNCH_ELL, base.a.mel, base.wobbling, wide_groups ? 16 : 8, 0,
                                      (int32_t)hyp.kind,
                                      base.c_max, base.H, base.SR, (int32_t)lds, base.a.n_reads, 1});
  return NVK_OK;
}
}  // namespace

int launch_ell(nvk_ctx *ctx, const DeviceModel &dm, const BatchArgs &a, int wobbling,
               const EllPlan &pl, const PlanTotals &tot, double *out_ll, int32_t *out_status, const EllHyp &hyp) {
  if (a.n_reads == 0) return NVK_OK;
  const int mel = a.mel;
  if (mel < 0 || mel > 4) {
    nvk_set_error("min_event_length %d outside the compiled range 0..4", mel);
    return NVK_ERR_UNSUPPORTED;
  }
  if (dm.k + 2 > 16) {
    nvk_set_error("k-mer size %d needs k + 2 = %d lanes per hypothesis, compiled limit is 16", dm.k, dm.k + 2);
    return NVK_ERR_UNSUPPORTED;
  }
  // (nvk_model_create builds no such table: the limit of the item code)
  const bool items = hyp.kind == EllKind::Joint || hyp.kind == EllKind::Edit;  // one packed item per hypothesis
  if (items && dm.alphabet > 8) {
    nvk_set_error("%s hypotheses pack a letter in 3 bits: alphabet %d, compiled limit is 8",
                  hyp.kind == EllKind::Joint ? "joint" : "edit", dm.alphabet);
    return NVK_ERR_UNSUPPORTED;
  }
  const bool wide_groups = dm.k + 2 > 8;  // 16 lanes per hypothesis instead of 8
  // rings sized by the largest skew of the batch that still fits 160 KB of LDS; a read beyond that gets
  // NVK_READ_TOO_WIDE and the others complete
  int H = 2, SR = 256;
  auto lds_for = [&](int cc) {
    H = cc + 1 < 2 ? 2 : cc + 1;
    SR = 256;
    while (SR < 64 * cc + CH) SR <<= 1;
    return (size_t)dens::ETN * 8 + (size_t)SR * 8 +
           (size_t)TABN * sizeof(SweepLane) + (size_t)H * 64 * 24 + 16;
  };
  int c = tot.max_c < 1 ? 1 : tot.max_c;
  while (c > 1 && lds_for(c) > 160 * 1024) c--;
  const size_t lds = lds_for(c);
  int per_cu = (int)((160 * 1024) / lds);
  if (per_cu > 12) per_cu = 12;
  if (per_cu < 1) per_cu = 1;
  int64_t slots = ctx->slots_override > 0 ? ctx->slots_override : (int64_t)ctx->num_cus * per_cu;
  if (slots > a.n_reads) slots = a.n_reads;
  // (Round 2 used no more slots than whole rounds of reads need — 10 000 reads: 4 rounds of 2 500 — because the
  // waves then end together; since the hypothesis loop issues a tenth fewer instructions the third wave per SIMD is
  // worth more than the even finish: 3 072 slots 105.5 ms, 2 500 slots 110.5 ms, 3 328 / 3 584 no better.)
  const int64_t half = (int64_t)(tot.max_W > 0 ? tot.max_W : 1) + 64;
  const int64_t stride = 2 * half;
  const int64_t cap = nvk_spill_cap(ctx, WS_SPILL);
  while (slots > 1 && slots * stride * (int64_t)sizeof(Cell) > cap) slots /= 2;
  int rc = nvk_ws_reserve(ctx, WS_SPILL, (size_t)slots * stride * sizeof(Cell));
  if (rc) return rc;
  rc = nvk_ws_reserve(ctx, WS_MISC, 256);
  if (rc) return rc;
  int *counter = (int *)ctx->ws[WS_MISC];
  NVK_HIP(hipMemsetAsync(counter, 0, sizeof(int), ctx->stream));

  EllArgs g;
  g.dm = dm;
  g.a = a;
  g.pl = pl;
  g.store = (Cell *)ctx->ws[WS_SPILL];
  g.store_stride = stride;
  g.half = half;
  g.n_reads = (int)a.n_reads;
  g.counter = counter;
  {
    int *order = nullptr;
    rc = launch_order(ctx, pl.metas, a.n_reads, nvk_plan_totals(ctx), &order, nullptr);  // (as launch_plan_ell left them)
    if (rc) return rc;
    g.order = order;
  }
  g.H = H;
  g.SR = SR;
  g.c_max = c;
  g.wobbling = wobbling;
  g.out_ll = out_ll;
  g.out_status = out_status;
  ctx->last_spill_bytes = (int64_t)tot.cells * 24 * 2;
  if (items) {
    if ((rc = nvk_ws_reserve(ctx, WS_JOINT, (size_t)(hyp.list.total_hyp + 1) * sizeof(int4)))) return rc;
  }
  switch (hyp.kind) {
    case EllKind::Full: return ell_dispatch<false, false, false>(ctx, g, hyp, wide_groups, slots, lds);
    case EllKind::Listed: return ell_dispatch<true, false, false>(ctx, g, hyp, wide_groups, slots, lds);
    case EllKind::Joint: return ell_dispatch<true, true, false>(ctx, g, hyp, wide_groups, slots, lds);
    case EllKind::Edit: return ell_dispatch<true, true, true>(ctx, g, hyp, wide_groups, slots, lds);
  }
  nvk_set_error("launch_ell: unknown hypothesis kind %d", (int)hyp.kind);
  return NVK_ERR_INVALID;
}
