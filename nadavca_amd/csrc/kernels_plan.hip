// Planner: per read, the band of every DP row, the per-row step densities gathered from
// the k-mer table, the lane-occupancy intervals and the wavefront skew.  One block per read.
//
// Reference behaviour restated here:
//   bands                 nadavca/dtw/dtw.cpp:7-35   (ComputeBandStarts / ComputeBandEnds)
//   row layout            nadavca/dtw/dtw.cpp:144-180 (transitions: 2R rows; else R+1)
//   k-mer id / densities  nadavca/dtw/kmer_model.cpp:22-94, sequence.cpp:6-29
// The expected-level gather (KmerModel::GetExpectedSignal, kmer_model.cpp:32-42) is the
// last kernel in this file.
#include <math.h>

#include "nvk_internal.h"
#include "kmer.h"
#include "lane3.h"
#include "wave.h"

namespace {

// What the reference leaves undefined and the C-ABI must refuse (sanitizers): a read whose
// slices leave the batch's arrays, an anchor outside the band rows, a base code that would index the
// k-mer table out of range (reference, both contexts).  `nthreads` threads of one block cooperate.
__device__ __forceinline__ int read_is_bad(const DeviceModel &dm, const BatchArgs &a, int rd, int tid,
                                           int nthreads) {
  const int64_t s0 = a.sig_off[rd], s1 = a.sig_off[rd + 1], r0 = a.ref_off[rd], r1 = a.ref_off[rd + 1];
  const int64_t a0 = a.anc_off[rd], a1 = a.anc_off[rd + 1];
  const int64_t b0 = a.cb_off[rd], b1 = a.cb_off[rd + 1], c0 = a.ca_off[rd], c1 = a.ca_off[rd + 1];
  const int64_t N64 = s1 - s0, R64 = r1 - r0;
  if (s0 < 0 || r0 < 0 || a0 < 0 || b0 < 0 || c0 < 0 || a1 < a0 || b1 < b0 || c1 < c0 ||
      s1 > a.total_signal || r1 > a.total_ref || a1 > a.total_anchors || b1 - b0 > 0x3fffffff ||
      c1 - c0 > 0x3fffffff)
    return 1;
  if (R64 < 1 || N64 < 1 || N64 > 0x3fffffff || R64 > 0x1fffffff) return 1;
  const int R = (int)R64, A = (int)(a1 - a0), nb = (int)(b1 - b0), na = (int)(c1 - c0);
  const int32_t *anc = a.anchors + 2 * a0;
  const int32_t *ref = a.reference + r0, *cb = a.ctx_before + b0, *ca = a.ctx_after + c0;
  int bad = 0;
  // anchors must name an existing band row (reference writes result[reference_index])
  for (int j = tid; j < A && !bad; j += nthreads) {
    int si = anc[2 * j], ri = anc[2 * j + 1];
    if (ri < 0 || ri > R || si < -(1 << 30) || si > (1 << 30)) bad = 1;
  }
  const unsigned alpha = (unsigned)dm.alphabet;
  for (int j = tid; j < R && !bad; j += nthreads)
    if ((unsigned)ref[j] >= alpha) bad = 1;
  for (int j = tid; j < nb && !bad; j += nthreads)
    if ((unsigned)cb[j] >= alpha) bad = 1;
  for (int j = tid; j < na && !bad; j += nthreads)
    if ((unsigned)ca[j] >= alpha) bad = 1;
  return bad;
}

// bands of the R+1 boundary rows (dtw.cpp:7-35): "later anchor overwrites", then prefix-max / suffix-min.  The
// `nthreads` threads of one block cooperate (tid = this thread).  tbs / tbe: R+1 scratch words each, LDS or global;
// bs / be: where the bands go, as int32 arrays of their own or (W = the scratch words' type, bs == tbs, be == tbe) in
// place, in the low words.  The two scans are independent: waves 0 and 1 run one each where the block has two waves.
template <class W>
__device__ __forceinline__ void plan_bands(const int32_t *anc, int A, int R, int N, int bw, unsigned long long *tbs,
                                           unsigned long long *tbe, W *bs, W *be, int tid, int nthreads) {
  const int lane = tid & 63, wv = tid >> 6;
  // scratch word = (anchor ordinal + 1) << 32 | payload ; atomicMax keeps the last anchor
  for (int j = tid; j <= R; j += nthreads) {
    tbs[j] = 0ull;
    tbe[j] = 0ull;
  }
  __syncthreads();
  for (int j = tid; j < A; j += nthreads) {
    int s = anc[2 * j], ri = anc[2 * j + 1];
    long long lo = (long long)s - bw;
    long long hi = (long long)s + bw;
    unsigned int vbs = (unsigned int)(lo > 0 ? lo : 0);  // max(0, s - bw)
    // min(N, s + bw); a negative value cannot be packed: clamp to -1 -> flagged as bad band
    unsigned int vbe = (unsigned int)((hi < N ? (hi < -1 ? -1 : hi) : N) + 1);
    unsigned long long tag = ((unsigned long long)(j + 1)) << 32;
    atomicMax(&tbs[ri], tag | vbs);
    atomicMax(&tbe[ri], tag | vbe);
  }
  __syncthreads();
  if (wv == 0) {
    int carry = 0;
    for (int base = 0; base <= R; base += 64) {
      int j = base + lane;
      int v = 0;
      if (j <= R) {
        unsigned long long w = tbs[j];
        v = (w >> 32) ? (int)(unsigned int)(w & 0xffffffffu) : 0;
      }
      v = max(wave_scan_max_dpp(v), carry);
      carry = __builtin_amdgcn_readlane(v, 63);
      if (j <= R) bs[j] = (W)(unsigned int)v;
    }
  }
  if (wv == (nthreads > 64 ? 1 : 0)) {
    int carry = N;
    for (int base = (R / 64) * 64; base >= 0; base -= 64) {
      int j = base + 63 - lane;  // descending rows over the lanes: the suffix minimum is a prefix scan
      int v = N;
      if (j <= R) {
        unsigned long long w = tbe[j];
        v = (w >> 32) ? (int)(unsigned int)(w & 0xffffffffu) - 1 : N;
      } else {
        v = 0x7fffffff;
      }
      v = min(wave_scan_min_dpp(v), carry);
      carry = __builtin_amdgcn_readlane(v, 63);
      if (j <= R) be[j] = (W)(unsigned int)v;
    }
  }
  __syncthreads();
}

// One block of PLAN_T threads per read.  What the planner keeps between its phases — the bands, the spans, the row
// offsets — is integers of one read.  The spans and offsets are functions of the bands, and the bands and the bases'
// k-mer ids are all that differs between reads: for a read of up to PLAN_BCAP band rows they stay in LDS
// (PlanStoreLds), for a longer one the bands go through global scratch and the ids are formed where they are used
// (PlanStoreGlobal).  plan_rows is the planner, written once over such a store.  The choice is per read, so it is
// uniform for the block and every wave takes every barrier.
constexpr int PLAN_T = 256;
constexpr int PLAN_VT = 2048;    // rows whose per-row offsets fit the LDS arrays (more: uniform offsets)
constexpr int PLAN_BCAP = 1024;  // band rows (R + 1) of a read planned in LDS

struct PlanShared {
  // x | S of the offsets (PLAN_VT ints each) and, for PlanStoreLds, bs, be (PLAN_BCAP ints each) behind them; the u64
  // tag|payload words of its bands, dead once bs / be are written, lie under x and S, which are born after them.
  unsigned long long pool[3 * PLAN_VT / 2];
  unsigned int ids[PLAN_BCAP];  // PlanStoreLds: the k-mer id of every base (ids below 2^32: plan_kernel)
  unsigned long long cells;
  int c, cw, var;
};
static_assert(2 * PLAN_BCAP * 8 <= 2 * PLAN_VT * 4 && 2 * PLAN_BCAP <= PLAN_VT, "LDS layout of PlanStoreLds");

// one read as the planner's phases see it
struct PlanRead {
  const int32_t *ref, *cb, *ca, *anc;
  int64_t r0;
  int N, R, A, T, nb, na, bw, mel;
};

// Where a read's bands and k-mer ids are.  bands(): plan_bands into the store, by the whole block; bs(j) / be(j): the
// band of boundary row j after it; fill_ids(first, stride): the threads that call it share the bases out, once, for
// kid(i), the k-mer id of base i (behind the next barrier).
struct PlanStoreLds {
  PlanShared &sh;
  __device__ __forceinline__ int *b() const { return (int *)sh.pool + 2 * PLAN_VT; }
  __device__ __forceinline__ void bands(const PlanRead &q, int tid) const {
    plan_bands(q.anc, q.A, q.R, q.N, q.bw, sh.pool, sh.pool + PLAN_BCAP, b(), b() + PLAN_BCAP, tid, PLAN_T);
  }
  __device__ __forceinline__ int bs(int j) const { return b()[j]; }
  __device__ __forceinline__ int be(int j) const { return b()[PLAN_BCAP + j]; }
  // A base's id serves its own row and, with transition rows, the two transition rows next to it, and the last phase
  // starts at the table gathers instead of at the reference loads.
  __device__ __forceinline__ void fill_ids(const DeviceModel &dm, const PlanRead &q, int first, int stride) const {
    for (int i = first; i < q.R; i += stride)
      sh.ids[i] = (unsigned int)kmer_id(dm, q.ref, q.R, q.cb, q.nb, q.ca, q.na, i);
  }
  __device__ __forceinline__ unsigned int kid(const DeviceModel &, const PlanRead &, int i) const { return sh.ids[i]; }
};
// per read 2*(R+1) u64 scratch words of bandtmp, the bands in their low words; nothing of the ids is kept, which is
// also the path of a table of 2^32 k-mers or more
struct PlanStoreGlobal {
  unsigned long long *tbs, *tbe;
  __device__ __forceinline__ void bands(const PlanRead &q, int tid) const {
    plan_bands(q.anc, q.A, q.R, q.N, q.bw, tbs, tbe, tbs, tbe, tid, PLAN_T);
  }
  __device__ __forceinline__ int bs(int j) const { return (int)(unsigned int)tbs[j]; }
  __device__ __forceinline__ int be(int j) const { return (int)(unsigned int)tbe[j]; }
  __device__ __forceinline__ void fill_ids(const DeviceModel &, const PlanRead &, int, int) const {}
  __device__ __forceinline__ int64_t kid(const DeviceModel &dm, const PlanRead &q, int i) const {
    return kmer_id(dm, q.ref, q.R, q.cb, q.nb, q.ca, q.na, i);
  }
};

// The planner of one read.  A row's integers are functions of the bands next to it and of its min event length (with
// transition rows: of its parity), so every phase takes them from the bands in the store:
//   bs, be   the band of the row's boundary
//   lo, hi   the lane's span: band + warm-up / pre-roll of the steps into and out of the row
//   off      sh_x / sh_S once the offsets are fixed
// The table constants are gathered once per row, in the last phase, which writes the row's RowParam and its two lane
// records; the constants of the row above come from the neighbouring lane.  Only the exact kernel (kernels_align.hip)
// reads the RowParam table — the sweeps of kernels_align3.hip take the lane records — so it is written on request
// (write_rows): a third of the phase's bytes, and that phase runs at the write rate of HBM.
template <class Store>
__device__ __forceinline__ void plan_rows(const Store st, const DeviceModel &dm, const PlanRead &q, int mode,
                                          double log_p_in, int c_cap, int rd, ReadMeta m, ReadMeta *metas,
                                          RowParam *rows, bool write_rows, Lane3 *lane_f, Lane3 *lane_r,
                                          int32_t *lane_offs, PlanShared &sh) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = q.N, T = q.T, mel = q.mel;
  const bool trans = (mode == PLAN_ALIGN_TRANS);
  constexpr int VT = PLAN_VT;
  int *sh_x = (int *)sh.pool, *sh_S = sh_x + VT;
  st.bands(q, tid);

  // min event length of step r -> r + 1 (RowParam::mel)
  auto rmel = [=](int r) { return (r + 1 < T && !(trans && (r & 1))) ? mel : 0; };
  auto BS = [=](int r) { return st.bs(trans ? (r + 1) >> 1 : r); };
  auto BE = [=](int r) { return st.be(trans ? (r + 1) >> 1 : r); };
  // forward lane of row r runs i = lo_r .. be_r, reverse lane i = hi_r .. bs_r  (see kernels_align.hip)
  auto LO = [=](int r) {
    int lo = BS(r);
    if (r > 0) {
      const int pm = rmel(r - 1);
      lo = min(lo, BS(r - 1) + pm) - max(pm - 1, 0);
    }
    return lo;
  };
  auto HI = [=](int r) {
    int hi = BE(r);
    if (r + 1 < T) {
      const int pm = rmel(r);
      hi = max(hi, BE(r + 1) - pm) + max(pm - 1, 0);
    }
    return hi;
  };

  // --- band checks, cell count and skew -----------------------------------------------------------------------
  // A lane starts its next row `idle` steps after it has left the previous one: the density of its first step
  // on the new row (and, with transition rows, the one its pair partner holds for the step after) was
  // evaluated with the old row's constants, and kernels_align3 lets those stale values pass through steps
  // on which the lane is outside its span instead of re-evaluating them at every row switch.
  const int idle = trans ? 2 : 1;
  int badband = 0;
  long long cells = 0;
  int cneed = 1;
  for (int r = tid; r < T; r += PLAN_T) {
    const int b0 = BS(r), b1 = BE(r);
    if (b1 < b0) badband = 1;
    cells += (long long)(b1 - b0 + 1);
    if (r >= 64) {
      int d = HI(r - 64) - LO(r) + idle;  // need 64*c > d
      if (d >= 0) cneed = max(cneed, d / 64 + 1);
    }
  }
  cneed = max(cneed, max(mel - 1, 1));
  badband = __syncthreads_or(badband);
  cells = wave_sum(cells);
  cneed = wave_max(cneed);
  if (lane == 0) {
    atomicAdd(&sh.cells, (unsigned long long)cells);
    atomicMax(&sh.c, cneed);
  }
  __syncthreads();
  const int c = sh.c;  // (sh.cells is complete too, and is read where the meta is written)
  // A band this wide for its row spacing (skew above the main launch's cap) is served by a TEAM of waves
  // (kernels_align3.hip): 64 * ALIGN3_TEAM_W lanes, one row each, so a lane's next row lies that many rows
  // on and the skew it needs is that of the row pair (r - 64 W, r) — on long reads with wide bands the band
  // moves on by more samples in 256 rows than it is wide, and the skew falls from ~28 to ~3.
  const bool team = (c > c_cap);
  int cw = 0;
  if (team) {
    constexpr int TL = 64 * ALIGN3_TEAM_W;
    if (tid == 0) sh.cw = max(mel - 1, 1);
    __syncthreads();
    int need = 1;
    for (int r = TL + tid; r < T; r += PLAN_T) {
      int d = HI(r - TL) - LO(r) + idle;  // need TL * cw > d
      if (d >= 0) need = max(need, d / TL + 1);
    }
    need = wave_max(need);
    if (lane == 0) atomicMax(&sh.cw, need);
    __syncthreads();
    cw = sh.cw;
  }

  // --- per-row time offsets (variable skew, used by kernels_align3.hip) ---------------------------
  // The uniform mapping t = i + c*r pays the worst pair of rows (r - 64, r) of the read on every row.
  // Here cell (r, i) is computed at step t = i + off[r] with the LEAST offsets that satisfy
  //   g[r] <= off[r] - off[r-1] <= c            (neighbour values wait at most c + mel steps in LDS)
  //   off[r] - off[r-64] >= hi[r-64] - lo[r] + 1 + idle  (a lane is free, and idle for `idle` steps, before its
  //                                                      next row starts)
  // (off[r] = c*r is one solution, so the least one exists and needs no more steps).  The lower bound
  // g[r] is what keeps the neighbour's value at least one step old, age = gap + mel >= 1: 1 for a row
  // fed without emission (mel 0), 1 - mel for a row fed by an emitting step — with transition rows the
  // two alternate, so a pair of rows needs no skew at all — and never so low that a row would start or
  // end before the row above it (the kernel's bookkeeping of the oldest open row relies on that order).
  // Without transition rows, and for min event lengths above 2, g[r] = max(mel - 1, 1).
  //
  // SWITCH ORDER.  The sweeps of kernels_align3.hip (one wave per read) serve a row switch as a scalar event
  // of the oldest open row, which needs the rows to be LEFT in row order: row r is left after step off[r] + BE(r)
  // (reverse sweep: before step off[r] + BS(r)), so
  //     off[r] - off[r-1] >= BE(r-1) - BE(r)   and   off[r] - off[r-1] >= BS(r-1) - BS(r)          (*)
  // must hold for every r.  It does, in every plan mode:
  //   - plan_bands makes the band starts a prefix maximum and the band ends a suffix minimum, so BS and BE are
  //     non-decreasing in r and the right-hand sides of (*) are <= 0 — also where the ends are flat, clipped to N
  //     or to 0 on many rows: equal ends leave in the order of the offsets;
  //   - the uniform offsets (teams, long reads, no fixed point) differ by c or cw >= 1;
  //   - the least offsets differ by at least g[r] (x is a prefix maximum, so non-decreasing), and the cap min(g, c)
  //     only ever lowers g to c >= 1.  g[r] >= 0 leaves nothing to show.  g[r] < 0 is possible only with transition
  //     rows at min event length 2, for an odd row r = 2k + 1 fed by the emitting step of row 2k: there
  //       HI(r-1) = max(be[k], be[k+1] - 2) + 1, HI(r) = be[k+1]  =>  HI(r-1) - HI(r) = max(be[k] - be[k+1] + 1, -1)
  //       LO(r-1) = bs[k], LO(r) = min(bs[k+1], bs[k] + 2) - 1    =>  LO(r-1) - LO(r) = max(bs[k] - bs[k+1] + 1, -1)
  //     and g[r] is at least both, i.e. at least BE(r-1) - BE(r) + 1 and BS(r-1) - BS(r) + 1.
  // tests/test_switch_order_cpu.py restates this on the host; the sweeps themselves hold a lane that is found past
  // its row's end at a rescale step to account (the read goes to the exact kernel).
  // With S[r] = g[1] + .. + g[r] and x[r] = off[r] - S[r] the first lower bound and the second are a
  // prefix maximum per block of 64 rows (the second's constant k[r] = hi[r-64] - lo[r] + 1 + idle - (S[r] - S[r-64])
  // is taken from the bands), and the upper bound is a suffix maximum of off[r] - c*r; both are iterated to
  // the fixed point by wave 0 (2-4 rounds on config-shaped reads).  Reads with more rows than the LDS arrays
  // hold, and team reads, keep the uniform offsets.
  const int gmin = max(mel - 1, 1);
  const bool neg_gaps = trans && mel <= 2;
  const bool fixp = !team && T <= VT && T > 64 && (neg_gaps || c > gmin);
  if (tid == 0) sh.var = 0;
  if (fixp) {
    for (int r = tid; r < T; r += PLAN_T) {
      int g = 0;
      if (r > 0) {
        g = gmin;
        if (neg_gaps) g = max(1 - rmel(r - 1), max(LO(r - 1) - LO(r), HI(r - 1) - HI(r)));
        g = min(g, c);
      }
      sh_S[r] = g;
      sh_x[r] = 0;
    }
  }
  __syncthreads();
  // The fixed point is wave 0's alone.  Beside it the other waves work out the k-mer id of every base, once, where
  // the store keeps them.
  const int t0 = fixp ? 64 : 0;
  if (tid >= t0) st.fill_ids(dm, q, tid - t0, PLAN_T - t0);
  {
    if (fixp && tid < 64) {  // S: inclusive prefix sum, block by block
      int carry = 0;
      for (int b0 = 0; b0 < T; b0 += 64) {
        const int r = b0 + lane;
        const int v = wave_scan_add_dpp(r < T ? sh_S[r] : 0) + carry;
        if (r < T) sh_S[r] = v;
        carry = __builtin_amdgcn_readlane(v, 63);
      }
      const int NEG = -0x20000000;
      bool changed = true;
      int iter = 0;
      while (changed && iter < 64) {
        changed = false;
        ++iter;
        int carry = 0;
        int xup = 0, Sup = 0;  // x and S of row r - 64: this lane's row of the previous block
        // (the next block's words are asked for ahead of this block's scan: a block's stores go to other rows)
        int cur_n = lane < T ? sh_x[lane] : NEG, Sr_n = lane < T ? sh_S[lane] : 0, d_n = 0;
        for (int b0 = 0; b0 < T; b0 += 64) {  // lower bounds, ascending
          const int r = b0 + lane;
          const int cur = cur_n, Sr = Sr_n, d = d_n;
          if (r + 64 < T) {
            cur_n = sh_x[r + 64];
            Sr_n = sh_S[r + 64];
            d_n = HI(r) - LO(r + 64) + 1 + idle;
          } else {
            cur_n = NEG;
            Sr_n = 0;
          }
          int v = cur;
          if (r < T && r >= 64) {
            const int k = d - (Sr - Sup);
            v = max(v, xup + k);
          }
          v = max(wave_scan_max_dpp(v), carry);
          if (r < T) {
            changed |= (v != cur);
            sh_x[r] = v;
          }
          carry = __builtin_amdgcn_readlane(v, 63);
          xup = v;
          Sup = Sr;
        }
        WAVE_SYNC();  // (the descending pass takes its rows on other lanes)
        int carryz = NEG;
        const int rz = ((T - 1) / 64) * 64 + 63 - lane;
        int curz_n = rz < T ? sh_x[rz] : 0, Sz_n = rz < T ? sh_S[rz] : 0;
        for (int b0 = ((T - 1) / 64) * 64; b0 >= 0; b0 -= 64) {  // gap limit, descending: rows over the lanes too
          const int r = b0 + 63 - lane;
          const int cur = curz_n;
          const int U = r < T ? c * r - Sz_n : 0;  // off[r] - c*r = x[r] - U[r]
          if (b0 >= 64) {
            curz_n = sh_x[r - 64];
            Sz_n = sh_S[r - 64];
          }
          int z = r < T ? cur - U : NEG;
          z = max(wave_scan_max_dpp(z), carryz);  // (the maximum over the rows from r up)
          if (r < T) {
            const int nx = z + U;
            changed |= (nx != cur);
            sh_x[r] = nx;
          }
          carryz = __builtin_amdgcn_readlane(z, 63);
        }
        WAVE_SYNC();
        changed = __any(changed);
      }
      if (lane == 0) sh.var = changed ? 0 : 1;  // not converged (never seen): uniform offsets
    }
    __syncthreads();
  }
  const bool var_ok = (sh.var != 0);
  const int x0 = var_ok ? sh_x[0] : 0;
  const int cu = team ? cw : c;  // uniform offsets
  auto OFF = [=](int r) { return var_ok ? sh_x[r] - x0 + sh_S[r] : cu * r; };

  // --- the row table and the lane records, one complete store per row ---------------------------------------------
  // A wave takes 63 consecutive rows on lanes 1..63; lane 0 gathers the constants of the row above them once more
  // and only hands them to lane 1, so the constants of row r - 1 are always one lane down.
  RowParam *rp = rows + m.row_off;
  const bool records = lane_f && !badband;
  const int top = T - 1;
  const int ST = cw ? 64 * ALIGN3_TEAM_W : 64;  // rows between a lane's consecutive rows (lane3.h)
  int plateau = 0;  // two adjacent bases with the same k-mer level (NVK_TIE_PLATEAU)
  for (int base = 0; base < T; base += 63 * (PLAN_T / 64)) {
    const int r = base + 63 * wv + lane - 1;
    const bool have = (r >= 0 && r < T);
    RowParam o;
    o.mean = 0.0;
    o.ac = 0.0;
    o.mc = 0.0;
    o.mel = 0;
    o.bs = o.be = o.lo = o.hi = o.off = 0;
    if (have && r + 1 < T) {
      if (trans && (r & 1)) {
        // transition step between base r/2 and r/2+1: constant log(0.01), -inf on equal means
        int i = r / 2;
        double m1 = dm.mean[st.kid(dm, q, i)];
        double m2 = dm.mean[st.kid(dm, q, i + 1)];
        o.ac = (m1 == m2) ? -INFINITY : log_p_in;
        plateau |= (m1 == m2) ? 1 : 0;
      } else {
        int i = trans ? r / 2 : r;
        const auto id = st.kid(dm, q, i);
        o.mean = dm.mean[id];
        o.ac = dm.ac[id];
        o.mc = dm.mc[id];
        o.mel = mel;
      }
    }
    RowParam p, nx;
    p.mean = __shfl_up(o.mean, 1, 64);
    p.ac = __shfl_up(o.ac, 1, 64);
    p.mc = __shfl_up(o.mc, 1, 64);
    p.bs = p.be = p.lo = p.hi = p.mel = p.off = 0;
    nx.mean = nx.ac = nx.mc = 0.0;
    nx.bs = nx.be = nx.lo = nx.hi = nx.mel = nx.off = 0;
    if (have && lane > 0) {
      o.bs = BS(r);
      o.be = BE(r);
      o.lo = LO(r);
      o.hi = HI(r);
      o.off = OFF(r);
      // (without transition rows: steps r - 1 and r are consecutive bases)
      if (!trans && r > 0 && r + 1 < T) plateau |= (p.mean == o.mean) ? 1 : 0;
      if (write_rows) rp[r] = o;
      if (records) {
        if (r > 0) {  // (lane3_row reads neither lo nor hi of the rows above and below)
          p.bs = BS(r - 1);
          p.be = BE(r - 1);
          p.mel = rmel(r - 1);
          p.off = OFF(r - 1);
        }
        if (r < top) {
          nx.bs = BS(r + 1);
          nx.be = BE(r + 1);
          nx.off = OFF(r + 1);
        }
        const int adv_f = (r >= ST) ? o.off - OFF(r - ST) : 0;
        const int adv_b = (r + ST <= top) ? OFF(r + ST) - o.off : 0;
        Lane3 f, b;
        lane3_row(o, p, r > 0, nx, r < top, N, adv_f, adv_b, f, b);
        (lane_f + m.row_off)[r] = f;
        (lane_r + m.row_off)[r] = b;
        (lane_offs + m.row_off)[r] = o.off;
      }
    }
  }
  plateau = __syncthreads_or(plateau);

  if (tid == 0) {
    const int hi_top = HI(T - 1);
    int t_min = LO(0);
    int t_max = hi_top + c * (T - 1);
    m.c = c;
    m.cw = cw;
    m.t_min = t_min;
    m.n_steps = t_max - t_min + 1;
    m.pad = hi_top + OFF(T - 1) - t_min + 1;  // steps under the per-row offsets ...
    // ... rounded up to a multiple of 32: kernels_align3 spills two steps per access, unrolls 8, rescales every
    // 16 and flushes its bit words every 32 steps, and with a whole number of each its loops need no end tests
    m.pad = (m.pad + 31) & ~31;
    m.cells = (long long)sh.cells;
    m.rsv = plateau ? 1 : 0;
    if (badband) m.status = NVK_READ_BAD_BAND;
    metas[rd] = m;  // (the batch totals: plan_totals_kernel)
  }
}

__global__ __launch_bounds__(PLAN_T, 5) void plan_kernel(DeviceModel dm, BatchArgs a, int mode,
                                                  double log_p_in, int c_cap, ReadMeta *metas,
                                                  RowParam *rows, unsigned long long *bandtmp,
                                                  Lane3 *lane_f, Lane3 *lane_r, int32_t *lane_offs, int write_rows) {
  // write_rows == 0: the RowParam table is left unwritten.  lane_f == null: no lane records — with write_rows that is
  // the rows-only pass.
  const int rd = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ PlanShared sh;
  if (rd >= a.n_reads) return;
  if (tid == 0) {
    sh.cells = 0ull;
    sh.c = 1;
  }
  const int64_t s0 = a.sig_off[rd], r0 = a.ref_off[rd], a0 = a.anc_off[rd];
  const int64_t N64 = a.sig_off[rd + 1] - s0;
  const int64_t R64 = a.ref_off[rd + 1] - r0;
  const int64_t A64 = a.anc_off[rd + 1] - a0;
  PlanRead q;
  q.nb = (int)(a.cb_off[rd + 1] - a.cb_off[rd]);
  q.na = (int)(a.ca_off[rd + 1] - a.ca_off[rd]);
  q.ref = a.reference + r0;
  q.cb = a.ctx_before + a.cb_off[rd];
  q.ca = a.ctx_after + a.ca_off[rd];
  q.anc = a.anchors + 2 * a0;
  q.r0 = r0;
  q.N = (int)N64;
  q.R = (int)R64;
  q.A = (int)A64;
  q.bw = a.bandwidth;
  q.mel = a.mel;

  ReadMeta m;
  m.sig_off = s0;
  m.ref_off = r0;
  m.N = q.N;
  m.R = q.R;
  m.status = NVK_READ_OK;
  m.pad = 0;
  m.cells = 0;
  m.cw = 0;
  m.rsv = 0;
  if (mode == PLAN_ALIGN_TRANS) {
    q.T = 2 * q.R;
    m.row_off = 2 * r0;
  } else {
    q.T = q.R + 1;
    m.row_off = r0 + rd;
  }
  m.T = q.T;
  m.c = 1;
  m.t_min = 0;
  m.n_steps = 0;

  int bad = read_is_bad(dm, a, rd, tid, PLAN_T);
  bad = __syncthreads_or(bad);
  if (bad) {
    m.status = NVK_READ_BAD_INPUT;
    if (tid == 0) metas[rd] = m;
    return;
  }
  if (q.R + 1 <= PLAN_BCAP && dm.n <= 0x100000000ll) {  // (PlanStoreLds keeps the k-mer ids as 32-bit words)
    plan_rows(PlanStoreLds{sh}, dm, q, mode, log_p_in, c_cap, rd, m, metas, rows, write_rows != 0, lane_f, lane_r,
              lane_offs, sh);
  } else {
    unsigned long long *tbs = bandtmp + 2 * (r0 + rd);
    plan_rows(PlanStoreGlobal{tbs, tbs + (q.R + 1)}, dm, q, mode, log_p_in, c_cap, rd, m, metas, rows,
              write_rows != 0, lane_f, lane_r, lane_offs, sh);
  }
}

// The batch totals of plan_kernel, reduced from the reads' metas.  (Every block of plan_kernel used to add its read
// to them itself: seven atomics on ONE cache line from each of 10 000 blocks are served one after the other, and
// those 0.7 ms were the kernel's run time whatever else it did.)  Here a block reduces 256 reads and adds once.
__global__ __launch_bounds__(256) void plan_totals_kernel(const ReadMeta *metas, int n, int c_cap, PlanTotals *totals) {
  const int rd = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int steps = 0, c = 0, cw = 0, T = 0, wide = 0;
  unsigned long long cells = 0ull, pad = 0ull;
  if (rd < n) {
    const ReadMeta m = metas[rd];
    if (m.status == NVK_READ_OK) {
      steps = max(m.n_steps, 0), c = max(m.c, 0), cw = max(m.cw, 0), T = max(m.T, 0);
      wide = (m.c > c_cap) ? 1 : 0;
      cells = (unsigned long long)m.cells;
      pad = (unsigned long long)m.pad;
    }
  }
  __shared__ int sh_i[4][5];
  __shared__ unsigned long long sh_u[4][2];
  steps = wave_max(steps), c = wave_max(c), cw = wave_max(cw), T = wave_max(T), wide = wave_sum(wide);
  cells = wave_sum(cells), pad = wave_sum(pad);
  if (lane == 0) {
    sh_i[wv][0] = steps, sh_i[wv][1] = c, sh_i[wv][2] = cw, sh_i[wv][3] = T, sh_i[wv][4] = wide;
    sh_u[wv][0] = cells, sh_u[wv][1] = pad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      steps = max(steps, sh_i[w][0]), c = max(c, sh_i[w][1]), cw = max(cw, sh_i[w][2]), T = max(T, sh_i[w][3]);
      wide += sh_i[w][4], cells += sh_u[w][0], pad += sh_u[w][1];
    }
    if (steps) atomicMax(&totals->max_steps, steps);
    if (c) atomicMax(&totals->max_c, c);
    if (cw) atomicMax(&totals->max_cw, cw);
    if (wide) atomicAdd(&totals->n_wide, wide);
    if (T) atomicMax(&totals->max_T, T);
    if (cells) atomicAdd(&totals->cells, cells);
    if (pad) atomicAdd(&totals->steps, pad);
  }
}


// ---------------------------------------------------------------------------------------------
// planner for estimate_log_likelihoods (dtw.cpp:37-131): bands, row-store offsets and the fused
// per-position descriptors of the prefix sweep and of the (mirrored) suffix sweep.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void plan_ell_kernel(DeviceModel dm, BatchArgs a, int wobbling,
                                                      EllPlan pl, unsigned long long *bandtmp,
                                                      PlanTotals *totals) {
  const int rd = blockIdx.x;
  const int lane = threadIdx.x;
  if (rd >= a.n_reads) return;
  const int64_t s0 = a.sig_off[rd], r0 = a.ref_off[rd], a0 = a.anc_off[rd];
  const int64_t N64 = a.sig_off[rd + 1] - s0;
  const int64_t R64 = a.ref_off[rd + 1] - r0;
  const int A = (int)(a.anc_off[rd + 1] - a0);
  const int nb = (int)(a.cb_off[rd + 1] - a.cb_off[rd]);
  const int na = (int)(a.ca_off[rd + 1] - a.ca_off[rd]);
  const int32_t *ref = a.reference + r0;
  const int32_t *cb = a.ctx_before + a.cb_off[rd];
  const int32_t *ca = a.ctx_after + a.ca_off[rd];
  const int32_t *anc = a.anchors + 2 * a0;
  const int N = (int)N64, R = (int)R64;

  ReadMeta m;
  m.sig_off = s0;
  m.ref_off = r0;
  m.row_off = r0;
  m.N = N;
  m.R = R;
  m.T = R;
  m.c = 1;
  m.t_min = 0;
  m.n_steps = 0;
  m.status = NVK_READ_OK;
  m.pad = 0;
  m.cells = 0;
  m.cw = 0;
  m.rsv = 0;

  int bad = read_is_bad(dm, a, rd, lane, 64);
  bad = __any(bad);
  if (bad) {
    m.status = NVK_READ_BAD_INPUT;
    if (lane == 0) pl.metas[rd] = m;
    return;
  }
  unsigned long long *tbs = bandtmp + 2 * (r0 + rd);
  unsigned long long *tbe = tbs + (R + 1);
  plan_bands(anc, A, R, N, a.bandwidth, tbs, tbe, tbs, tbe, lane, 64);

  int32_t *bs = pl.bs + r0 + rd, *be = pl.be + r0 + rd, *rowoff = pl.rowoff + r0 + rd;
  int badband = 0;
  int carry = 0;
  for (int base = 0; base <= R; base += 64) {
    int r = base + lane;
    int w = 0;
    if (r <= R) {
      int b0 = (int)(unsigned int)tbs[r], b1 = (int)(unsigned int)tbe[r];
      bs[r] = b0;
      be[r] = b1;
      w = b1 - b0 + 1;
      if (w < 1) {
        badband = 1;
        w = 0;
      }
    }
    // exclusive prefix sum of the row widths
    const int inc = wave_scan_add(w, lane);
    if (r <= R) rowoff[r] = carry + inc - w;
    carry += __shfl(inc, 63, 64);
  }
  badband = __any(badband);
  const int cells = carry;
  __syncthreads();

  FusedParam *fw = pl.fwd + r0, *rv = pl.rev + r0;
  for (int j = lane; j < R; j += 64) {
    FusedParam f;
    f.has_wob = (j > 0 && wobbling) ? 1 : 0;
    int64_t id = kmer_id(dm, ref, R, cb, nb, ca, na, j);
    f.b_mean = dm.mean[id];
    f.b_ac = dm.ac[id];
    f.b_mc = dm.mc[id];
    f.wbs = bs[j];
    f.wbe = be[j];
    f.ebs = bs[j + 1];
    f.ebe = be[j + 1];
    f.store_off = rowoff[j + 1];
    fw[j] = f;
    // suffix sweep, lane jj handles boundary i = R - jj: input suffix[i] (band i), wobble with the
    // mixture of k-mers (i, i-1), emit with k-mer i-1 into suffix[i-1] (band i-1); mirrored i' = N - i
    const int jj = j, i = R - jj;
    FusedParam g;
    g.has_wob = (i < R && wobbling) ? 1 : 0;
    id = kmer_id(dm, ref, R, cb, nb, ca, na, i - 1);
    g.b_mean = dm.mean[id];
    g.b_ac = dm.ac[id];
    g.b_mc = dm.mc[id];
    g.wbs = N - be[i];
    g.wbe = N - bs[i];
    g.ebs = N - be[i - 1];
    g.ebe = N - bs[i - 1];
    g.store_off = rowoff[i - 1];
    rv[jj] = g;
  }
  __syncthreads();
  int cneed = 1;
  for (int j = 64 + lane; j < R; j += 64) {
    int d1 = fw[j - 64].ebe - fw[j].wbs;
    int d2 = rv[j - 64].ebe - rv[j].wbs;
    int d = max(d1, d2);
    if (d >= 0) cneed = max(cneed, d / 64 + 1);
  }
  int c = wave_max(cneed);
  if (lane == 0) {
    m.c = c;
    m.cells = cells;
    m.n_steps = N + 1 + c * R;
    if (badband) m.status = NVK_READ_BAD_BAND;
    pl.metas[rd] = m;
    if (!badband) {
      atomicMax(&totals->max_steps, m.n_steps);
      atomicMax(&totals->max_c, c);
      atomicMax(&totals->max_T, R);
      atomicMax(&totals->max_W, cells);
      atomicAdd(&totals->cells, (unsigned long long)cells);
      atomicAdd(&totals->steps, (unsigned long long)m.n_steps);
    }
  }
}


__global__ void expected_kernel(DeviceModel dm, int64_t n_reads, int64_t total_ref,
                                const int32_t *reference, const int64_t *ref_off,
                                const int32_t *cbs, const int64_t *cb_off, const int32_t *cas,
                                const int64_t *ca_off, double *out) {
  // one thread per base
  int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total_ref) return;
  const int64_t rd = owner_of(ref_off, n_reads, g);
  int R = (int)(ref_off[rd + 1] - ref_off[rd]);
  int nb = (int)(cb_off[rd + 1] - cb_off[rd]);
  int na = (int)(ca_off[rd + 1] - ca_off[rd]);
  int pos = (int)(g - ref_off[rd]);
  // a base code outside the alphabet in the k-mer's window (kmer.h): the level is reported as NaN
  const int32_t *ref = reference + ref_off[rd], *cb = cbs + cb_off[rd], *ca = cas + ca_off[rd];
  const int64_t id = kmer_id_checked(dm, ref, R, cb, nb, ca, na, pos);
  out[g] = id >= 0 ? dm.mean[id] : (double)NAN;
}


// ---------------------------------------------------------------------------------------------
// Longest-first work order.  Persistent waves take whole reads from a counter; when read lengths
// differ, the launch ends with the waves that happened to start a long read last.  Handing the reads
// out longest first (64 buckets of the step count, descending, original order inside a bucket up
// to the race of the fill) bounds that tail by the shortest reads instead.
// ---------------------------------------------------------------------------------------------
constexpr int ORD_B = 64;        // step-count buckets per launch class
constexpr int ORD_N = 2 * ORD_B;  // two classes: reads swept by teams of waves first, then the one-wave reads
// Class-major: each class of launch_align3 then serves one contiguous range of launch positions, so its chunks,
// spill slots and workgroups count only the reads it sweeps (a few wide reads in a batch of narrow ones used
// to cost every read a team-sized slot).  Reads without a plan (bad input / band) go last.
__device__ __forceinline__ int order_bucket(const ReadMeta &m, int max_steps) {
  if (m.status != NVK_READ_OK) return ORD_N - 1;
  long long b = (long long)m.n_steps * ORD_B / ((long long)max_steps + 1);
  const int sb = ORD_B - 1 - (int)(b < 0 ? 0 : (b > ORD_B - 1 ? ORD_B - 1 : b));
  return (m.cw != 0 ? 0 : ORD_B) + sb;
}
// (max_steps comes from the planner's totals ON THE DEVICE: the order is built behind the planner without a host
// round trip in between)
// Both kernels count in LDS first: an atomicAdd per read on a handful of bucket counters in global memory is served
// one read after the other (the same-address effect of DESIGN.md 5.3, item 1); a block's reads meet in its own LDS
// counters and the block then goes to global memory once per bucket it holds reads of.
__global__ __launch_bounds__(256) void order_count_kernel(const ReadMeta *metas, int n, const PlanTotals *tot,
                                                          int *cnt) {
  __shared__ int lc[ORD_N];
  for (int b = threadIdx.x; b < ORD_N; b += blockDim.x) lc[b] = 0;
  __syncthreads();
  const int rd = blockIdx.x * blockDim.x + threadIdx.x;
  if (rd < n) atomicAdd(&lc[order_bucket(metas[rd], tot->max_steps)], 1);
  __syncthreads();
  for (int b = threadIdx.x; b < ORD_N; b += blockDim.x)
    if (lc[b]) atomicAdd(&cnt[b], lc[b]);
}
__global__ void order_scan_kernel(int *cnt) {  // one wave, two buckets per lane: cnt[b] -> first position of bucket b; cnt[ORD_N+b] = 0
  int lane = threadIdx.x;
  const int v0 = cnt[2 * lane], v1 = cnt[2 * lane + 1], s = wave_scan_add(v0 + v1, lane);
  cnt[2 * lane] = s - v0 - v1;
  cnt[2 * lane + 1] = s - v1;
  cnt[ORD_N + 2 * lane] = 0;
  cnt[ORD_N + 2 * lane + 1] = 0;
}
// steps_out (or null): the steps of the reads in the order they are handed out (sizes the per-read spill slots of
// kernels_align3.hip)
// A block reserves one range per bucket (cnt[ORD_N + b]: the bucket's positions handed out so far) and places its
// reads in it by their rank among the block's reads of that bucket.
__global__ __launch_bounds__(256) void order_fill_kernel(const ReadMeta *metas, int n, const PlanTotals *tot, int *cnt,
                                                         int *order, int32_t *steps_out) {
  __shared__ int lc[ORD_N];  // the block's reads per bucket, then the first position of its range
  for (int b = threadIdx.x; b < ORD_N; b += blockDim.x) lc[b] = 0;
  __syncthreads();
  const int rd = blockIdx.x * blockDim.x + threadIdx.x;
  ReadMeta m;
  int b = 0, rank = 0;
  if (rd < n) {
    m = metas[rd];
    b = order_bucket(m, tot->max_steps);
    rank = atomicAdd(&lc[b], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < ORD_N; k += blockDim.x)
    if (lc[k]) lc[k] = cnt[k] + atomicAdd(&cnt[ORD_N + k], lc[k]);
  __syncthreads();
  if (rd < n) {
    const int pos = lc[b] + rank;
    order[pos] = rd;
    if (steps_out) steps_out[pos] = (m.status == NVK_READ_OK) ? m.pad : 0;
  }
}

__global__ void count_flags_kernel(const int32_t *flags, int64_t n, int32_t *out) {
  int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int f = (g < n) ? flags[g] : 0;
  // (three counts of at most 2^20 each would fit one word; kept apart for n up to 2^31)
  int v = ((f & 7) != 0) ? 1 : 0, v0 = f & 1, v1 = (f >> 1) & 1, v2 = (f >> 2) & 1;  // (bit 3, the plateau mark, is not a tie class)
  v = wave_sum(v), v0 = wave_sum(v0), v1 = wave_sum(v1), v2 = wave_sum(v2);
  if ((threadIdx.x & 63) == 0 && v) {
    atomicAdd(out, v);
    if (v0) atomicAdd(out + 1, v0);
    if (v1) atomicAdd(out + 2, v1);
    if (v2) atomicAdd(out + 3, v2);
  }
}

}  // namespace

int launch_count_flags(nvk_ctx *ctx, const int32_t *flags, int64_t n, int32_t *out_count) {
  NVK_HIP(hipMemsetAsync(out_count, 0, 4 * sizeof(int32_t), ctx->stream));
  if (n <= 0) return NVK_OK;
  hipLaunchKernelGGL(count_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, flags, n,
                     out_count);
  NVK_HIP(hipGetLastError());
  return NVK_OK;
}

// order[0..n) = read indices, longest (by step count) first; `order` lives in ctx->ws[WS_ORDER]
int launch_order(nvk_ctx *ctx, const ReadMeta *metas, int64_t n_reads, const PlanTotals *tot_dev, int **order,
                 int32_t *steps_out) {
  *order = nullptr;
  if (n_reads <= 0) return NVK_OK;
  int rc = nvk_ws_reserve(ctx, WS_ORDER, (size_t)n_reads * sizeof(int) + 2 * ORD_N * sizeof(int));
  if (rc) return rc;
  int *ord = (int *)ctx->ws[WS_ORDER];
  int *cnt = ord + n_reads;
  NVK_HIP(hipMemsetAsync(cnt, 0, 2 * ORD_N * sizeof(int), ctx->stream));
  const unsigned blocks = (unsigned)((n_reads + 255) / 256);
  TimerScope ts(ctx, NVK_K_PLAN);
  hipLaunchKernelGGL(order_count_kernel, dim3(blocks), dim3(256), 0, ctx->stream, metas, (int)n_reads, tot_dev, cnt);
  hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(64), 0, ctx->stream, cnt);
  hipLaunchKernelGGL(order_fill_kernel, dim3(blocks), dim3(256), 0, ctx->stream, metas, (int)n_reads, tot_dev, cnt, ord,
                     steps_out);
  NVK_HIP(hipGetLastError());
  *order = ord;
  return NVK_OK;
}

int launch_plan(nvk_ctx *ctx, const DeviceModel &dm, const BatchArgs &a, int mode,
                ReadMeta *metas, RowParam *rows, unsigned long long *bandtmp, PlanTotals *totals,
                void *lane_f, void *lane_r, int32_t *lane_offs, int write_rows,
                const std::function<int()> *meanwhile) {
  // totals == null: a second pass over a planned batch (the rows-only pass), whose totals stand
  if (totals) NVK_HIP(hipMemsetAsync(totals, 0, sizeof(PlanTotals), ctx->stream));
  if (a.n_reads == 0) return meanwhile ? (*meanwhile)() : NVK_OK;
  int rc = NVK_OK;
  {
    TimerScope ts(ctx, NVK_K_PLAN);
    // the transition constant comes from the host libm, like the model's ac/mc (kmer_model.cpp:77)
    const double log_p_in = log(0.01);
    hipLaunchKernelGGL(plan_kernel, dim3((unsigned)a.n_reads), dim3(PLAN_T), 0, ctx->stream, dm, a, mode,
                       log_p_in, ALIGN1_C_CAP, metas, rows, bandtmp, (Lane3 *)lane_f, (Lane3 *)lane_r, lane_offs,
                       write_rows);
    if (totals)
      hipLaunchKernelGGL(plan_totals_kernel, dim3((unsigned)((a.n_reads + 255) / 256)), dim3(256), 0, ctx->stream,
                         metas, (int)a.n_reads, ALIGN1_C_CAP, totals);
    // the caller's host work that needs nothing of the plan: the planner is the first long kernel of a batch, and
    // what the host does here it does not do between the planner's end and the first sweep.  (Behind stop(): with
    // timing on the scope's end waits for the kernels, and fills queued here stay out of the timed interval.)
    ts.stop();
    if (meanwhile) rc = (*meanwhile)();
  }
  NVK_HIP(hipGetLastError());
  return rc;
}

int launch_plan_ell(nvk_ctx *ctx, const DeviceModel &dm, const BatchArgs &a, int wobbling,
                    const EllPlan &pl, unsigned long long *bandtmp, PlanTotals *totals) {
  NVK_HIP(hipMemsetAsync(totals, 0, sizeof(PlanTotals), ctx->stream));
  if (a.n_reads == 0) return NVK_OK;
  {
    TimerScope ts(ctx, NVK_K_PLAN);
    hipLaunchKernelGGL(plan_ell_kernel, dim3((unsigned)a.n_reads), dim3(64), 0, ctx->stream, dm, a,
                       wobbling, pl, bandtmp, totals);
  }
  NVK_HIP(hipGetLastError());
  return NVK_OK;
}

int launch_expected(nvk_ctx *ctx, const DeviceModel &dm, int64_t n_reads, int64_t total_ref,
                    const int32_t *reference, const int64_t *ref_off, const int32_t *cb,
                    const int64_t *cb_off, const int32_t *ca, const int64_t *ca_off, double *out) {
  if (total_ref == 0) return NVK_OK;
  {
    TimerScope ts(ctx, NVK_K_EXPECTED);
    unsigned blocks = (unsigned)((total_ref + 255) / 256);
    hipLaunchKernelGGL(expected_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dm, n_reads,
                       total_ref, reference, ref_off, cb, cb_off, ca, ca_off, out);
  }
  NVK_HIP(hipGetLastError());
  return NVK_OK;
}
