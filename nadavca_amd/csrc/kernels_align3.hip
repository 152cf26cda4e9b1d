// refine_alignment v3 on gfx950: plain doubles under a wave-uniform running scale.
//
// Same mathematics, mapping and memory layout as kernels_align.hip (one row per lane, one read per
// wave, systolic anti-diagonal wavefront, suffix spill in (step, lane) order, one update bit per
// cell instead of a back-pointer) — read that file's header first.  What changes is the number
// representation, which is where most of that kernel's instructions went:
//
//   kernels_align.hip keeps every probability as (double mantissa, int32 exponent) and pays
//   ldexp/frexp/max/select chains and a third register per value for it.  But all values a wave
//   touches in one step lie on one anti-diagonal of the band, i.e. within a few hundred bits of
//   each other.  So here a value is a PLAIN double, stored as  true * 2^L(u)  with ONE running
//   log-scale L per wave and step, kept in scalar registers.  Every RS steps the wave looks at its
//   largest live exponent and moves L so that it sits at 2^TARGET; the move is applied by adding
//   the shift to the exponent of that step's densities (an integer add on a value that is being
//   ldexp'ed anyway), and a neighbour value from D steps ago is brought to the current scale by
//   the (scalar) sum of the shifts of those D steps — zero on most steps, so the ldexp is skipped.
//   Scaling by powers of two is exact, so as long as nothing leaves the double range the integer
//   results are those of the exact kernel.  Range guards, per read: a value above 2^900 or NaN (tested at
//   the rescale steps; in between an inf or NaN reaches the row sums below); a
//   scale move that had to be capped (the wave's largest value collapsed faster than the scale can
//   follow); and the ROW MASS — every allowed path crosses every row exactly once, so the posterior
//   mass sum_i prefix[r][i] * suffix[r][i] is the same number for every row, and a flushed cell
//   that mattered shows up as a row whose sum deviates.  A flagged read is re-run by the exact
//   kernel (status NVK_READ_RETRY_INTERNAL, never visible to callers).
//
//   Path DP: scores of one row only ever meet scores of the same row (running maximum, arg-max)
//   or are handed to the next row, so scores are (double, integer scale) pairs: the running maximum
//   is kept normalised (mantissa in [0.5,1), scale G), an incoming score is shifted onto that scale
//   before the comparison, and G travels with the score — which is all the tie tolerance of
//   xm::gt_tol needs.  The comparison itself is path_step.h: the margin of gt_tol, best * |G| * 2^-52, is a function
//   of the maximum and is formed only in the block the wave enters when some lane's pair lies inside the 2^-24 tie
//   margin; everywhere else "greater by more than the margin" and "greater" are the same bit as long as |G| < 2^27
//   (the lemma in that header).  A row moves |G| by at most 1024, so reads of up to 2^17 rows are below that bound
//   whatever their data; longer ones go to the exact kernel, and so does, as one more range guard, a read in which
//   a lane leaves a row with |G| >= 2^26.  The last row's arg-max is treated the same way.
//
// Memory: spill 8 B per cell (+4 B of scale per RS steps) instead of 12 B per cell; no row table in LDS
// (lane3_kernel prepares per-sweep lane records, a lane fetches the record of its next row through the scalar
// cache when it switches rows), so 9.5 KB of LDS per wave.  Launches (launch_align3): the reverse sweeps of all
// reads of a chunk, then their forward sweeps (template parameter PHASE: 73 and 115 registers, 24 and 16
// waves per CU), every read with a spill slot of its own; reads are handed to the persistent waves longest
// first (launch_order); reads whose band is too wide for one wave's rings (skew above ALIGN1_C_CAP) are swept
// by teams of four waves (template parameter W, ReadMeta::cw) in a second pair of launches.  The rescale period
// is compiled in (template parameter RSH): 14 kernels per min event length, the ones a launch can reach
// (select_sweeps).
//
// Time mapping: cell (r, i) is computed at step t = i + off[r] with the planner's per-row offsets
// (RowParam::off, kernels_plan.hip) instead of one skew per read; a lane record carries the age of the
// neighbour's value (gap to the row it receives from + mel, at least 1; the gap itself may be -1 for a
// row fed by an emitting step) and the row's advance over the lane's previous row.  A value that is D
// steps old missed the scale moves of its last D steps, the emission product carries those of its
// last mel steps: the correction applied to their product is ([age < D] - [age < mel]) * last move.
//
// What the step does NOT do any more (each was measured): no masks on loaded or
// computed values — a lane reads a permanent zero entry of the history ring wherever it is outside its
// own span or the predecessor cell is outside the predecessor's band (one interval per row,
// Lane3::pA/pW), which keeps its own recurrence at zero by itself, and the spilled suffix is zero
// outside the band, so the posterior is; no vector address arithmetic for the spill (buffer resource:
// scalar step offset + constant lane offset) or for the history ring (read index advanced per lane,
// write address = scalar slot base + constant lane offset); the emission product's row-type select is
// one FMA with per-row constants; uniform conditions live in scalar registers; no loop end tests (the step
// count is a multiple of 32) and, with 16 steps per loop trip and the rescale period compiled in, no test on
// the step's position in the period (a period of 32 steps: on the trip's parity); the two rare cases "first
// row" / "last row" behind one scalar test; the signal ring's refill loaded one chunk ahead; no density
// re-evaluation at a row switch (the planner keeps the lane idle for the steps on which stale densities
// pass); no tie margin carried from update to update (five vector instructions of every step, three of them at the
// FP64 rate, and two registers: path_step.h) and no copy of the score's scale for the rare first-row case (row 0's
// lane keeps G = 0 by itself); no trip through the LDS crossbar for the wave's largest exponent at the rescale steps
// (wave_max_i, wave.h: six DPP maxima and a v_readlane where a butterfly of six ds_bpermute_b32 was, each waited
// for); with one wave per read no vector test for "some lane is past its row" on every step and no ballot loop over
// the lanes that are — the rows are left in row order (SWITCH ORDER, kernels_plan.hip), so the step compares the
// oldest open row's sample index with its band end as two scalars and the block serves that row's lane, with no
// per-lane masks carried through it ("an emitting lane switched" is the served lane's parity, "first row" / "last row"
// / the oldest open row come from the scalar row counter, the bound on G travels with the row mass), no search for
// the oldest open row, and no wait right behind the record's scalar loads (unconditional, index clamped, the record
// made inert where the lane gets no row: the row's bookkeeping runs under their latency); a lane found past its row's
// end at a rescale step sends the read to the exact kernel.  (The teams keep the ballot form: changing that block
// made a lockstep step slower.)
// Tried and not kept (DESIGN.md 5.1 and 5.1a have the measurements): 32 forward steps per trip (128 registers),
// the sample of the next density read one step earlier, update bits shifted in with v_addc, the history-ring
// read pipelined one step ahead with age-1 values by DPP, lane records prefetched into L2, 5 waves per SIMD in
// the forward sweep, the first prefetch loads in step order (a wait by count on every even step instead of one
// drain per trip), the reverse sweep's scale word loaded one period ahead.
#include <math.h>

#include <new>
#include <vector>

#include "nvk_internal.h"
#include "xmath.h"
#include "dens.h"
#include "lane3.h"
#include "path_step.h"
#include "wave.h"

namespace {

using dens::density;
using dens::density_begin;
using dens::density_end;
using dens::DensHalf;
using dens::ETN;

constexpr int CH = 64;      // signal refill chunk (samples): one per lane
static_assert(CH == 64, "a refill is one sample per lane");
constexpr int PF = 8;       // forward sweep: spill prefetch depth (steps)
constexpr int RU = 16;      // reverse sweep: steps per loop trip
// forward sweep: steps per loop trip, a multiple of the prefetch depth (16: with the compiled-in rescale period
// of 16 the step's position in the period is static; measured 8 -> 16: -2.3 %, 32: slower again — 128 registers)
constexpr int FT = 16;
static_assert(FT % PF == 0 && 32 % FT == 0, "forward trip");
static_assert(32 % PF == 0 && PF % 2 == 0 && 32 % RU == 0 && RU % 2 == 0, "the step count is a multiple of 32 (kernels_plan.hip)");
// rescale period: 2^RSH steps (template parameter RSH, 8, 16 or 32); must exceed c + mel so that at most one
// rescale lies inside the window a neighbour value travels through
using path_step::GBIG;  // scale of an empty running maximum (see the path step)
// Largest upward move per rescale.  When the wave's largest value collapses by more than this within one
// period (only off-path cells live, or a sharp model on a noisy signal) the running scale cannot follow
// without sending the next densities' exponents out of range; the move is capped (no inf / NaN is ever
// produced) and the read is handed to the exact kernel — capping silently was tried and is WRONG: the
// values that flush then can decide the path search although every row sum still checks out
// (tests/dev/fuzz_parity.py seed 11, iteration 4230).
constexpr int DMAX = 1000;  // the density exponent (<= ~3) plus the move must stay inside the double range
                            // (1000: a long read's reverse sweep ends in far-off-path cells that collapse by
                            // ~28 bits per step — 906 bits in a 32-step period on BASELINE config 5 reads)
constexpr int TARGET = 250; // exponent the largest live value is moved to
#define HUGE_V 0x1.0p+900
#define MASS_TOL 1e-9          // allowed relative spread of the rows' posterior mass
static_assert(path_step::TIE_BITS == NVK_TIE_BITS && path_step::TIE_ULPS == NVK_TIE_ULPS, "path_step.h restates xmath.h's tie margins");
static_assert(path_step::TIE_EXACT == NVK_TIE_EXACT && path_step::TIE_NEAR == NVK_TIE_NEAR && path_step::TIE_ULP == NVK_TIE_ULP, "path_step.h restates the tie classes");

// The spill is addressed through a buffer resource: address = resource base (scalar) + scalar byte
// offset of the step + per-lane byte offset (a constant vector register), so neither the store of the
// reverse sweep nor the prefetch of the forward sweep needs vector address arithmetic.
// Two consecutive steps travel together: 16 bytes per lane and access (8-byte accesses reach little more
// than half of the HBM rate 16-byte ones do, MI355X_MICROARCH.md; measured here: the spill traffic in
// 8-byte pieces cost a quarter of the kernel's time).  Pair p holds steps 2p and 2p+1 of the FORWARD
// order, [pair][lane][2]; the planner makes the step count even so that the reverse sweep, which runs the
// steps downwards, ends on a pair boundary.
// Both carry the non-temporal bit (`nt` in the assembly): a batch's spill, 25 GB per 10 000 config-2 reads, is
// written once and read once, far beyond L2 and the Infinity Cache, so nothing is lost by streaming it past them,
// and a line it does not displace is one of the lane records, the signal or the bit words (measured, DESIGN.md
// 5.1a: reverse launch -3.5 %, forward launch -1.2 %).  Nothing is handed over inside a launch, so no
// write-through form is wanted.
constexpr int SPILL_AUX = 2;  // the builtins' cache-policy argument: bit 1 = nt on gfx950
typedef int v4i_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void spill_store2(__amdgpu_buffer_rsrc_t rs, int lane16, int pair, double v_even,
                                             double v_odd) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i_t, make_double2(v_even, v_odd)), rs, lane16,
                                         pair * 1024, SPILL_AUX);
}
__device__ __forceinline__ double2 spill_load2(__amdgpu_buffer_rsrc_t rs, int lane16, int pair) {
  return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, pair * 1024, SPILL_AUX));
}

// end of a step: the history ring's writes of this step before the next step's reads.  A team of waves
// (W > 1) meets at a workgroup barrier behind a wait for its LDS operations ONLY — __syncthreads() would
// also wait for the spill stores / the spill prefetch in flight, which is the traffic the step overlaps.
#define STEP_SYNC()                                                              \
  do {                                                                           \
    if (W == 1) WAVE_SYNC();                                                     \
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");         \
  } while (0)
// around a refill of the wave's own signal ring (inside wave-uniform, not team-uniform, control flow)
#define RING_SYNC()                 \
  do {                              \
    if (W == 1) __syncthreads();    \
    else WAVE_SYNC();               \
  } while (0)

struct Align3Args {
  const ReadMeta *metas;
  const Lane3 *fwdl;
  const Lane3 *revl;
  const int32_t *offs;  // per-row time offsets, [row]
  const double *signal;
  double *spill_v;   // suffix values, [slot][step][lane], scaled by 2^L(step)
  int32_t *spill_L;  // [slot][reverse step / RS] running log-scale of the reverse sweep
  uint32_t *bp;      // path update bits, [slot][step/32][lane]
  int64_t spill_stride;  // cells per slot
  int64_t L_stride;      // ints per slot
  int64_t bp_stride;     // words per slot
  int n_reads;
  int *counter;
  const int *order;  // reads in the order they are handed out (longest first), or null
  int H, SR;
  int transitions;
  int c_cap;        // this launch serves reads with c <= c_cap (its class's skew: ReadMeta::c or ::cw)
  int flag_above;   // ... and hands reads with c > c_cap to the exact kernel (last launch only)
  int2 *rstate;      // per read (K, suspect) handed from the reverse launch to the forward one
  int read_lo;       // positions [read_lo, read_lo + n_reads) of `order` are served, the spill of
                     // position p lives in slot p - read_lo
  int *n_retry;      // reads handed to the exact kernel
  int32_t *ties;     // per read: NVK_TIE_EXACT | NVK_TIE_NEAR — a path comparison fell inside the tie margin (nvk_last_tie_flags)
  int32_t *out_events;
  int32_t *out_status;
};

// (also sets the lane's read index into the history ring: the neighbour's value is D = gap + mel
// steps old, i.e. in slot (su - D) mod H)
#define TAKE_LANE(l)                                                                   \
  do {                                                                                 \
    if (!PAIR || em) { mean = (l).mean; ac2 = (l).ac; mc2 = (l).mc; }  /* (a transition lane keeps its partner's) */ \
    melr = (l).mg & 15;                                                                \
    D = ((l).mg >> 4) & 255;                                                           \
    bs = (l).bs; pA = (l).pA; pW = (l).pW;                                             \
    ra = (int)min((unsigned)(su - D), (unsigned)(su - D + H)) * TL + nb;               \
    if (!PAIR) { pm = melr ? 1.0 : 0.0; qm = melr ? 0.0 : 1.0; }                       \
    if (PAIR && !em) cq = (shift_now != 0) ? ldexp((l).mean, shift_now) : (l).mean;    \
  } while (0)

// The record of a lane's next row comes through the SCALAR cache when the lane switches rows (lanes that
// switch in the same step are served one after the other; the row number is uniform then).  A vector load
// here — this kernel prefetched the record one row ahead into registers — has to be waited for with the
// vector-memory counter, and vector-memory operations complete in order: that wait drained every spill
// store (reverse sweep) or spill prefetch (forward sweep) issued before it, at every row switch of any
// lane, i.e. every ~7 steps (measured by ablation: a fifth of the kernel's time).  Scalar loads have a
// counter of their own, and the 12 registers per lane the prefetched record occupied are free.
__device__ __forceinline__ Lane3 lane3_sload(const Lane3 *p) {
  typedef const __attribute__((address_space(4))) v4i_t *cptr_t;
  cptr_t q = (cptr_t)(uintptr_t)p;
  const v4i_t q0 = q[0], q1 = q[1], q2 = q[2];
  Lane3 l;
  l.mean = __hiloint2double(q0.y, q0.x);
  l.ac = __hiloint2double(q0.w, q0.z);
  l.mc = __hiloint2double(q1.y, q1.x);
  l.bs = q1.z; l.end = q1.w;
  l.lo = q2.x; l.pA = q2.y; l.pW = q2.z; l.mg = q2.w;
  return l;
}

// exchange with the other lane of the pair (2m, 2m+1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ int pair_swap(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true); }
__device__ __forceinline__ double pair_swap(double v) {
  return __hiloint2double(pair_swap(__double2hiint(v)), pair_swap(__double2loint(v)));
}

template <int MEL>
__device__ __forceinline__ double emission_product(double e, double e1, double e2, double e3) {
  double P = 1.0;  // newest first, as the reference multiplies (node_next_row.h:27-29,51-53)
  if (MEL >= 1) P = e;
  if (MEL >= 2) P = P * e1;
  if (MEL >= 3) P = P * e2;
  if (MEL >= 4) P = P * e3;
  return P;
}

// running scale: L(u) = L(u-1) + delta_u; delta is nonzero only on rescale steps
struct Scale {
  int L;        // current log-scale
  int d_last;   // shift applied at the last rescale step (every RS steps; may be 0)
  int d_next;   // shift of the NEXT step (densities are computed one step ahead)
};

// RSH: log2 of the rescale period, 3, 4 or 5 (launch_align3 picks it: the shortest period of at least 16
// steps, 8 without transition rows, that exceeds c + mel).  Compiled in, it folds the tests on the step's
// position in the period away.  It divides 32 and so the step count (kernels_plan.hip pads
// it to a multiple of 32): the reverse sweep's rescale steps, counted from the read's other end, fall on the
// forward sweep's own.  (The team bands that need a period of 32 steps ran a form with the period taken from
// the launch arguments; it can be rebuilt from commit db75295.)
//
// PAIR (model_transitions): emitting rows and transition rows alternate, so lanes 2m and 2m+1 always hold
// one of each (64 is even: a lane's rows keep their parity).  A transition row's density is a constant,
// so its lane has nothing to evaluate — it evaluates for its partner instead: on odd steps the emitting
// lane evaluates its density of the next step and the partner that of the step after next (with the
// emitting lane's row constants and sample index, refreshed by DPP whenever some lane changes rows); on
// even steps nothing is evaluated and the two exchange their `e` registers (one DPP swap).  The
// transition lane's own density enters its recurrence as e_eff = fma(e, pm, cq) with per-lane constants
// (pm, cq) = (1, 0) on emitting lanes and (0, the row's constant times this step's scale move) on the
// others — no select.  One density evaluation per lane and TWO steps instead of one per step.
//
// PHASE: 1 / 2 — two launches: the reverse sweeps of ALL reads of a chunk, then their forward sweeps, every read
// with a spill slot of its own (25 GB for 10 000 config-2 reads: what 288 GB of HBM are for).  The memory
// system then sees a pure write stream followed by a pure read stream instead of a mix (measured with
// tools/ubench_spill.hip in this access shape: 5.5 and 5.7-6.2 TB/s against 4.3 TB/s mixed), and the
// reverse sweep — no path search, half the registers — runs with 6 waves per SIMD instead of 4 (one launch,
// both sweeps per wave, was measured and not kept: DESIGN.md 5).  Launch bounds, waves per SIMD:
constexpr int LB = 4;           // forward sweep
constexpr int LB_REV = 7;       // (72 registers allowed; config 2's kernel takes 70 and has no scratch since wave_max_i went the DPP way; 6.45 against 6.59 ms at 6)
constexpr int LB_REV_TEAM = 6;  // (the team's reverse sweep: 80 registers; 5 and 4 measured the same within noise)
//
// W: waves per read.  1 — the mapping above.  W > 1 (wide bands: ReadMeta::cw != 0) — a
// TEAM of W waves sweeps one read with one row per lane of its TL = 64 W lanes: a lane's next row lies TL
// rows on, so the skew a band of given width needs falls roughly W-fold (and with it the history ring per
// lane, i.e. LDS per wave: BASELINE config 5 reads need skew ~28 and 57 KB of LDS with one wave — 2 waves
// per CU — and skew 3 and 10 KB per wave with four).  The history ring is shared by the team ([slot][team
// lane]; the value of lane 63 of one wave goes to lane 0 of the next), everything else stays per wave: its
// own signal ring and refill bookkeeping, its own spill region and bit words, its own row switches.  The
// team moves in lockstep — one workgroup barrier per step (STEP_SYNC) — and shares ONE running scale:
// every wave posts its largest exponent one step before the rescale step and all take the maximum.  The
// ring has one slot more than the oldest age read (c + mel + 1): within one wave "read the oldest slot,
// then overwrite it" is program order, across waves it would be a race.
template <int MEL, int RSH, bool PAIR, int PHASE, int W>
__global__ __launch_bounds__(64 * W, PHASE == 1 ? (W > 1 ? LB_REV_TEAM : LB_REV) : LB) void align3_kernel(Align3Args g) {
  constexpr int TL = 64 * W;  // lanes of the team
  constexpr int RS = 1 << RSH;  // rescale period (steps)
  static_assert(32 % RS == 0, "the period must divide the step count, a multiple of 32 (kernels_plan.hip, m.pad)");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int gl = threadIdx.x;  // lane of the team
  const int wv = (W > 1) ? __builtin_amdgcn_readfirstlane(gl >> 6) : 0;
  double *etab = reinterpret_cast<double *>(smem);
  double *ring = etab + ETN + (size_t)wv * g.SR;               // the wave's own signal ring
  double *hist = etab + ETN + (size_t)W * g.SR;                 // reverse sweep: suffix values
  double2 *hist2 = reinterpret_cast<double2 *>(hist);          // forward sweep: (prefix, path score)
  // entry H*64 of both arrays is a permanent zero: a lane whose predecessor cell lies outside the
  // predecessor's band reads it instead of masking what it read (one select on the index instead of
  // one per loaded register)
  // (the reverse-only launch keeps 8 bytes per lane and slot: its zero entry is hist[H*64])
  int *ghist = reinterpret_cast<int *>(hist2 + (size_t)g.H * TL + 1);
  int *s_read = (PHASE == 1) ? reinterpret_cast<int *>(hist + (size_t)g.H * TL + 1) : ghist + (size_t)g.H * TL + 1;
  // team exchange: every wave's largest exponent (rescale), its flags, and the last row's arg-max
  int *tmax = s_read + 2, *tflag = tmax + W, *tfidx = tflag + W;

  const int lane = gl & 63;
  const int H = g.H, RM = g.SR - 1;
  uint32_t *bp = g.bp + (size_t)blockIdx.x * g.bp_stride;

  for (int q = gl; q < W * g.SR; q += TL) etab[ETN + q] = 0.0;
  dens::fill_table(etab, gl, TL);
  const int HZ = H * TL;
  if (gl == 0) {
    if (PHASE == 1) {
      hist[HZ] = 0.0;
    } else {
      hist2[HZ] = make_double2(0.0, 0.0);
      ghist[HZ] = 0;
    }
  }
  // per-lane constants kept in vector registers (the compiler would otherwise rebuild them from scalars
  // with one or two VOP3 instructions at every use): byte offsets of the lane inside a history slot and
  // the indices of the zero entry
  unsigned char *histb = reinterpret_cast<unsigned char *>(hist2);
  unsigned char *ghistb = reinterpret_cast<unsigned char *>(ghist);
  int gl16 = gl * 16, gl8 = gl * 8, HZv = HZ, HZ2v = (PHASE == 1) ? HZ : 2 * HZ;
  asm volatile("" : "+v"(gl16), "+v"(gl8), "+v"(HZv), "+v"(HZ2v));
  const int lane16 = (W == 1) ? gl16 : lane * 16;  // the lane's offset inside a step of the wave's spill

  while (true) {
    __syncthreads();
    if (gl == 0) *s_read = atomicAdd(g.counter, 1);
    __syncthreads();
    const int pos0 = __builtin_amdgcn_readfirstlane(*s_read);
    if (pos0 >= g.n_reads) break;
    const int pos = pos0 + g.read_lo;
    const int rd = g.order ? g.order[pos] : pos;
    const ReadMeta m = g.metas[rd];
    if (m.status != NVK_READ_OK) {
      if (PHASE == 2 && gl == 0) g.out_status[rd] = m.status;
      continue;
    }
    if ((W > 1) != (m.cw != 0)) continue;  // served by the other launch (one wave per read / a team)
    const int cm = (W > 1) ? m.cw : m.c;
    if (cm > g.c_cap) {           // band too wide for this launch's LDS rings
      if (PHASE == 2 && g.flag_above && gl == 0) {
        g.out_status[rd] = NVK_READ_RETRY_INTERNAL;
        atomicAdd(g.n_retry, 1);
      }
      continue;
    }
    // the read's own spill slot
    // (0x00020000: raw 32-bit data format, no swizzle; the range check is left wide open — the slot's size
    // bounds every offset by construction)
    const size_t slot = (size_t)pos0;
    const __amdgpu_buffer_rsrc_t spill_rs = __builtin_amdgcn_make_buffer_rsrc(
        g.spill_v + (slot * W + wv) * g.spill_stride, 0, 0x7ffffff0, 0x00020000);
    int32_t *spill_L = g.spill_L + slot * g.L_stride;
    const int T = __builtin_amdgcn_readfirstlane(m.T);
    const int N = __builtin_amdgcn_readfirstlane(m.N);
    const int c = __builtin_amdgcn_readfirstlane(cm);
    const int t_min = __builtin_amdgcn_readfirstlane(m.t_min);
    const int n_steps = __builtin_amdgcn_readfirstlane(m.pad);  // steps under the per-row offsets
    const int t_max = t_min + n_steps - 1;
    const Lane3 *fwdl = g.fwdl + m.row_off;
    const Lane3 *revl = g.revl + m.row_off;
    const int32_t *offs = g.offs + m.row_off;  // cell (r, i) is computed at step t = i + offs[r]
    const double *sig = g.signal + m.sig_off;
    const int top = T - 1;
    int K = 0;          // true exponent of the largest suffix[0][.]
    bool suspect = false;  // something left the double range: the exact kernel must redo this read

    // =========================== reverse sweep: suffix rows -> spill ===========================
    if (PHASE == 1) {
      int r = top - ((top - gl) & (TL - 1));
      // Lanes without a row keep bs = hi = -big: never active, never finished.  For the other
      // rows `hi` already folds the "predecessor column exists" test (i + mel <= N).
      double mean = 0, ac2 = 0, mc2 = 0;
      int bs = -0x40000000, hi = -0x40000000, pA = 0x40000000, pW = 0, melr = 0, D = 1;
      double pm = 0.0, qm = 1.0;
      // PAIR: emitting lanes of the reverse sweep are the even ones (row r applies step r -> r+1)
      const bool em = PAIR ? ((lane & 1) == 0) : true;
      double cq = 0.0;   // PAIR: the transition lane's own (constant) density times this step's scale move
      int ia = 0;        // PAIR: sample index of the lane's next density evaluation
      int dsel = 0;      // PAIR: scale move applied by that evaluation (emitting lanes, rescale steps only)
      int shift_now = 0; // scale move of the current step (uniform)
      if (PAIR) { pm = em ? 1.0 : 0.0; qm = em ? 0.0 : 1.0; }
      int su = 0;                       // history slot written at this step
      const int nb = (gl + 1) & (TL - 1);   // the lane the values come from
      int ra = (H - 1) * TL + nb;       // read index into the history ring, advanced with su
      bool is_init = false;
      int i = t_max;
      if (r >= 0) {
        const Lane3 cu = revl[r];
        TAKE_LANE(cu);
        hi = cu.end;
        is_init = (r == top);
        i = t_max - offs[r];
      }
      double prev = 0.0, e1 = 1.0, e2 = 1.0, e3 = 1.0;
      double o_hold = 0.0;  // the value of the even step of a trip, stored together with the odd step's
      int kmax = -0x40000000;
      int r_old = (W == 1) ? top : max(wave_max_i(r), -1);  // the oldest open row of this wave
      // sample index of the oldest open row (scalar); no row at all: a value no refill test reaches
      int i_old = (r_old >= 0) ? __builtin_amdgcn_readlane(i, r_old & 63) : 0x40000000;
      // (one wave per read) the band start of that row, where its lane leaves it: read with i_old when r_old moves
      int e_old = (r_old >= 0) ? __builtin_amdgcn_readlane(bs, r_old & 63) : -0x40000000;
      int filled_lo = (i_old / CH + 1) * CH;
      while (i_old - 3 < filled_lo) {
        filled_lo -= CH;
        for (int q = lane; q < CH; q += 64) {
          int idx = filled_lo + q;
          ring[idx & RM] = (idx >= 0 && idx < N) ? sig[idx] : 0.0;
        }
      }
      // the chunk below the filled ones, loaded one refill ahead: a refill then writes a value that arrived long
      // ago instead of waiting for a fresh load (and, with it, for every spill access in flight)
      double nxt;
      {
        const int idx = filled_lo - CH + lane;
        nxt = (idx >= 0 && idx < N) ? sig[idx] : 0.0;
      }
      __syncthreads();
      Scale sc{0, 0, 0};
      int sh_until = 0;  // (scalar) steps below this one still see values from before the last scale move
      // (pair_swap only ever under full exec, never inside a conditional operand: a DPP read of a
      // disabled lane returns 0)
      const int ip0 = PAIR ? pair_swap(i) : 0;
      if (PAIR) {  // the partner's row constants and sample index (see the row switch below)
        const double pmn = pair_swap(mean), pac = pair_swap(ac2), pmc = pair_swap(mc2);
        if (!em) { mean = pmn; ac2 = pac; mc2 = pmc; }
        // step 0 is even: the transition lane holds its partner's density of step 1, sample s[ip - 1]
        ia = em ? i : ip0 - 1;
      } else {
        ia = i;
      }
      double e = density(ring[ia & RM], mean, ac2, mc2, 0, etab);
      if (PAIR) ia = (em ? i - 1 : ip0 - 2) - 1;  // first evaluation at step 1
      int init_live = 1;  // (uniform, a scalar register) the last row is still being swept
      int row0_live = (__builtin_amdgcn_readfirstlane(r) == 0) ? 1 : 0;  // lane 0 is on row 0

      // RU steps per trip (as the forward sweep does with its prefetch depth): loop overhead and the tests on
      // the step's position in the rescale period fold away (measured: 2 -> 8 steps -4.8 %, 16 another 1 %); the loop-carried
      // registers rotate by renaming instead of by copies
      for (int ub = 0; ub < n_steps; ub += RU) {
#pragma unroll
      for (int uq = 0; uq < RU; uq++) {
        const int u = ub + uq;  // (n_steps is a multiple of 32, kernels_plan.hip: no end test inside a trip)
        const int t = t_max - u;
        // this step's shift was decided at the end of the previous one
        const int age = u & (RS - 1);  // steps since the last rescale step (the scale only moves there)
        if (age == 0 && u > 0) {
          sc.L += sc.d_next;
          sc.d_last = sc.d_next;
          sh_until = (sc.d_next != 0) ? u + c + MEL : 0;
          sc.d_next = 0;
          if (PAIR) { cq = ldexp(cq, sc.d_last); dsel = 0; }  // (0 stays 0 on emitting lanes)
        }
        if (PAIR && age == 1 && u > 1) cq = ldexp(cq, -sc.d_last);  // exact: the constant is back
        shift_now = (age == 0 && u > 0) ? sc.d_last : 0;
        if constexpr (W == 1) {
          // The row switch as a scalar event (one wave per read).  The rows are left in row order (SWITCH ORDER,
          // kernels_plan.hip), so the lane that leaves its row next is the one that holds the oldest open row: the
          // step compares two scalars and the block serves "while the oldest open row is past its start".  What
          // the ballot form carried per lane — "took a new row", "first row" — follows from the row counter.
          if (i_old < e_old) {
            int sw_em = 0;  // (scalar) an emitting lane has taken a new row: the served lane's parity
            do {
              const int fl = r_old & 63;
              const int rn = r_old - 64;  // the row that lane takes
              // (unconditional, index clamped: the bookkeeping below runs under the load's latency)
              Lane3 nx = lane3_sload(revl + max(rn, 0));
              // No row left for that lane (rn < 0): the clamped record made inert — never inside a span (pA, pW: the
              // lane's values stay zero whatever its other fields say) and never past its start (the guard at the
              // rescale steps).  As a mask behind the compiler's back: written as a condition it becomes a branch
              // that takes the load, and the wait for it, along.
              const int nm = __builtin_amdgcn_readfirstlane(rn) >> 31;
              nx.bs = (nx.bs & ~nm) | (-0x40000000 & nm);
              nx.pA = (nx.pA & ~nm) | (0x40000000 & nm);
              nx.pW &= ~nm;
              if (lane == fl) {
                r = rn;
                prev = 0.0;
                i += nx.mg >> 12;
                TAKE_LANE(nx);
                hi = nx.end;
              }
              if (PAIR) sw_em |= ~nm & (fl ^ 1);  // (bit 0: the reverse sweep's emitting lanes are the even ones)
              r_old -= 1;
              // (no open row left: a sample index neither this test nor a refill test ever reaches; both lanes
              // read, then chosen: a conditional v_readlane is a branch)
              const int io = __builtin_amdgcn_readlane(i, r_old & 63), eo = __builtin_amdgcn_readlane(bs, r_old & 63);
              i_old = (r_old >= 0) ? io : 0x40000000;
              e_old = (r_old >= 0) ? eo : -0x40000000;
            } while (i_old < e_old);
            if (PAIR) {  // see the team's form below
              if (sw_em & 1) {
                const double pmn = pair_swap(mean), pac = pair_swap(ac2), pmc = pair_swap(mc2);
                const int ip = pair_swap(i);
                if (!em) { mean = pmn; ac2 = pac; mc2 = pmc; }
                ia = (em ? i - 1 : ip - 2) - ((u & 1) ? 0 : 1);
              }
            }
            // (from the row counter, as sign bits: r_old == top; 0 <= r_old < 64)
            unsigned blk = (unsigned)r_old >> 6;
            blk = (unsigned)__builtin_amdgcn_readfirstlane((int)blk);
            init_live = (int)((unsigned)(top - r_old - 1) >> 31);
            row0_live = (int)((blk - 1u) >> 31);
          }
        } else {
        bool fin = (i < bs);
        if (__any(fin)) {
          bool redo = false;  // this lane has taken a new row
          for (unsigned long long fm = __builtin_amdgcn_ballot_w64(fin); fm != 0; fm &= fm - 1) {
            const int fl = __builtin_ctzll(fm);
            const int rn = __builtin_amdgcn_readlane(r, fl) - TL;  // (uniform) the row that lane takes
            Lane3 nx;
            nx.mean = nx.ac = nx.mc = 0.0; nx.bs = nx.end = nx.lo = nx.pA = nx.pW = nx.mg = 0;
            if (rn >= 0) nx = lane3_sload(revl + rn);
            if (lane == fl) {
              r = rn;
              i += nx.mg >> 12;
              prev = 0.0;
              if (r >= 0) {
                TAKE_LANE(nx);
                hi = nx.end;
                is_init = false;
                redo = true;
              } else {
                hi = -0x40000000; bs = -0x40000000; pA = 0x40000000; pW = 0;
                if (PAIR && !em) cq = 0.0;
              }
            }
          }
          if (PAIR) {
            // when an EMITTING lane has switched: every transition lane takes its partner's (possibly
            // new) row constants and sample index.  The densities in flight — the emitting lane's `e` of
            // this step and, on an even step, the one its partner holds for the next step — were evaluated
            // with the OLD row's constants and are NOT evaluated again: the planner keeps a lane outside
            // its new row's span for two steps after a switch (one without transition rows), so they are
            // multiplied into zeros (kernels_plan.hip, `idle`; re-evaluating them here was a dependent
            // LDS -> table -> polynomial chain inside every switch of an emitting lane).  (A transition
            // lane's own switch changes nothing about the densities.)
            if (__any(redo && em)) {
              const double pmn = pair_swap(mean), pac = pair_swap(ac2), pmc = pair_swap(mc2);
              const int ip = pair_swap(i);
              if (!em) { mean = pmn; ac2 = pac; mc2 = pmc; }
              const int odd = u & 1;
              if (W > 1) {  // (teams: re-evaluated as before — measured 4 % faster there: a lockstep step is as
                            // long as its longest chain, and this block's code shapes the compiler's schedule)
                redo = em ? redo : !odd;
                if (redo) e = density(ring[(em ? i : ip - 1) & RM], mean, ac2, mc2, em ? shift_now : 0, etab);
              }
              ia = (em ? i - 1 : ip - 2) - (odd ? 0 : 1);
            }
          } else if (W > 1 && redo) {
            e = density(ring[i & RM], mean, ac2, mc2, shift_now, etab);
          }
          while (r_old >= 0 && __builtin_amdgcn_readlane(r, r_old & 63) != r_old)
            r_old -= (W > 1 && (r_old & 63) == 0) ? 1 + 64 * (W - 1) : 1;  // (the wave's rows only)
          // (no open row left: a sample index no refill test ever reaches)
          i_old = (r_old >= 0) ? __builtin_amdgcn_readlane(i, r_old & 63) : 0x40000000;
          init_live &= (__builtin_amdgcn_readlane(r, top & 63) == top) ? 1 : 0;
          row0_live = (__builtin_amdgcn_readfirstlane(r) == 0) ? 1 : 0;
        }
        }
        {
          // (a younger row may be one sample beyond the oldest one; PAIR: and its partner evaluates one
          // sample further ahead)
          const int need_min = i_old - (PAIR ? 3 : 2);
          while (need_min < filled_lo) {
            filled_lo -= CH;
            RING_SYNC();
            ring[(filled_lo + lane) & RM] = nxt;
            {
              const int idx = filled_lo - CH + lane;
              nxt = (idx >= 0 && idx < N) ? sig[idx] : 0.0;
            }
            RING_SYNC();
          }
        }
        // LDS reads first: the neighbour's value and the sample of the next step's density
        // the neighbour's value is D = gap + mel steps old: slot (su - D) mod H
        // outside the predecessor's band: the zero entry
        const int hs = ((unsigned)(i - pA) <= (unsigned)pW) ? ra : HZ2v;
        const bool evalstep = !PAIR || (uq & 1);  // (static) PAIR: densities are evaluated on odd steps
        double xn = 0.0;
        if (evalstep) xn = ring[(PAIR ? ia : i - 1) & RM];
        const double pv = hist[hs];
        // scalar shifts that bring a neighbour value from D steps ago to the current scale
        // a rescale lies between the step a neighbour value was produced at and now?  (rare, uniform)
        const bool sh_any = (u < sh_until);
        DensHalf dn;
        if (evalstep) dn = density_begin(xn, mean, ac2, mc2, etab);
        // ---- the cell (r, i): out = P * pred[i + mel] + e(s[i]) * out[i + 1]
#define ACTIVE_R ((i <= hi) && (i >= bs))
        double P = emission_product<MEL>(e, e1, e2, e3);
        if (MEL > 0) P = fma(P, pm, qm);  // (1, 0) on emitting rows, (0, 1) on rows without emission: P or 1
        double t1 = P * pv;
        if (sh_any) {  // the value missed the moves of its last D steps; P carries those of the last mel
          asm volatile("");
          t1 = ldexp(t1, ((age < D) ? sc.d_last : 0) - ((age < melr) ? sc.d_last : 0));
        }
        const double ee = PAIR ? fma(e, pm, cq) : e;  // the transition lane's own density is its constant
        double o = fma(ee, prev, t1);  // zero outside the lane's span, see Lane3::pA
        // Cells far off the likely path are thousands of bits below the wave's largest value and
        // flush to zero here; that cannot change any value that matters (their contributions are
        // below 2^-53 of it in exact arithmetic too).  Overflow / NaN must never happen.
        if (init_live | row0_live) {  // (one scalar test for the two rare cases: the first and the last row)
          asm volatile("");
          if (init_live) {
            // (one wave per read: the lane's row number says it; a team carries the flag as before)
            if ((W == 1) ? (r == top) : is_init) o = ACTIVE_R ? ldexp(1.0, sc.L) : 0.0;
          }
          if (row0_live) {  // row 0 lives on lane 0; only its kmax is read
            if (o != 0.0) kmax = max(kmax, __builtin_amdgcn_frexp_exp(o) - sc.L);
          }
        }
        prev = o;
        *reinterpret_cast<double *>(histb + (su * (8 * TL) + gl8)) = o;
        // (n_steps is even: an odd u is the even step 2p of the forward order, the step before it 2p + 1)
        if (uq & 1) {
          spill_store2(spill_rs, lane16, (t - t_min) >> 1, o, o_hold);
        } else {
          o_hold = o;
        }
        if (age == 0) {  // the scale only moves on these steps
          asm volatile("");  // (a scalar branch first: the lane test need not run at every step)
          if (gl == 0) spill_L[u >> RSH] = sc.L;
        }
        // ---- rescale decision for the next step, then the next step's density
        if (W > 1 && age == RS - 2) {  // team: the waves' largest exponents meet one step ahead
          const int mxw = wave_max_i((o != 0.0) ? __builtin_amdgcn_frexp_exp(o) : -0x40000000);
          if (lane == 0) tmax[wv] = mxw;
        }
        if (age == RS - 1) {
          // (range guard of the values themselves: here only — an inf or NaN between two rescale steps
          // reaches the posterior sums of its row and fails the row-mass check)
          suspect |= !(o <= HUGE_V);
          // (the switch order's guard: a lane still on a row it is past was not the oldest one when it left)
          if (W == 1) suspect |= (i < bs);
          int mx;
          if (W == 1) {
            mx = wave_max_i((o != 0.0) ? __builtin_amdgcn_frexp_exp(o) : -0x40000000);
          } else {
            mx = tmax[0];
#pragma unroll
            for (int w = 1; w < W; w++) mx = max(mx, tmax[w]);
            mx = __builtin_amdgcn_readfirstlane(mx);
          }
          sc.d_next = (mx > -0x40000000) ? min(TARGET - mx, DMAX) : 0;
          // (a capped move matters to the step it is applied to: after the sweep's last step — the padding
          // behind row 0, where only cells off the band are alive and collapse — there is none)
          suspect |= (u + 1 < n_steps) && (mx > -0x40000000) && (TARGET - mx > DMAX);
          if (PAIR) dsel = em ? sc.d_next : 0;  // (RS - 1 is odd: an evaluation step)
        }
        i -= 1;
        i_old -= 1;
        e3 = e2; e2 = e1; e1 = e;
        if (!PAIR) {
          e = density_end(dn, sc.d_next);
        } else if (evalstep) {
          e = density_end(dn, dsel);  // emitting lane: its next step; partner: the step after next
          ia -= 2;
        } else {
          e = pair_swap(e);  // the emitting lane takes what its partner evaluated one step ago
        }
        su = (su + 1 == H) ? 0 : su + 1;
        ra = (int)min((unsigned)(ra + TL), (unsigned)(ra + TL - HZ));
        STEP_SYNC();
      }
      }
      K = __builtin_amdgcn_readfirstlane(kmax);
      if (K == -0x40000000) K = 0;
    }
    if (PHASE == 1) {  // hand K and the range guard's verdict to the forward launch
      bool any_s = __any(suspect);
      if (W > 1) {  // (row 0, and so K, lives in wave 0)
        if (lane == 0) tflag[wv] = any_s ? 1 : 0;
        __syncthreads();
        int fl = 0;
#pragma unroll
        for (int w = 0; w < W; w++) fl |= tflag[w];
        any_s = (fl != 0);
      }
      if (gl == 0) g.rstate[rd] = make_int2(K, any_s ? 1 : 0);
      continue;
    }
    if (PHASE == 2) {
      const int2 rs = g.rstate[rd];
      K = __builtin_amdgcn_readfirstlane(rs.x);
      suspect = (rs.y != 0) || (T > path_step::PATH_ROWS_PROVEN);  // (path_step.h, the bound)
    }
    __syncthreads();  // (also drains the stores)
    __builtin_amdgcn_s_dcache_inv();

    // ================= forward sweep: prefix rows, posterior, path DP, update bits =================
    // arg-max of the last row: best score, its margin, its scale, its cell (in registers: kept in LDS, read
    // and written by the last row's lane only, it cost 4 % — one more LDS round trip on that row's steps)
    double fbest = 0.0;
    int fidx = -1, fG = 0;
    // (scalar) lanes that saw a comparison inside the tie margin, by class (include/nadavca_hip.h): the two scores
    // exactly equal (amb_x), different but within NVK_TIE_ULPS margins of xm::gt_tol — ulps of the reference's
    // log value, where its own rounding may decide — (amb_u), beyond that but inside 2^-24 relative (amb_n)
    unsigned long long amb_x = 0, amb_u = 0, amb_n = 0;
    {
      int r = gl;
      // Lanes without a row keep lo = be = +big: never active, never finished.  For the other rows
      // `lo` already folds the "predecessor column exists" test (i - mel >= 0).
      double mean = 0, ac2 = 0, mc2 = 0;
      int bs = 0, be = 0x40000000, lo = 0x40000000, pA = 0x40000000, pW = 0, melr = 0, D = 1;
      double pm = 0.0, qm = 1.0;
      // PAIR: emitting lanes of the forward sweep are the odd ones (row r applies step r-1 -> r)
      const bool em = PAIR ? ((lane & 1) != 0) : true;
      double cq = 0.0;
      int ia = 0, dsel = 0, shift_now = 0;  // see the reverse sweep
      if (PAIR) { pm = em ? 1.0 : 0.0; qm = em ? 0.0 : 1.0; }
      int su = 0;
      const int nb = (gl - 1) & (TL - 1);
      int ra = (H - 1) * TL + nb;
      bool is_init = false;
      int i = t_min - 64 * c;
      if (r < T) {
        const Lane3 cu = fwdl[r];
        TAKE_LANE(cu);
        be = cu.end; lo = cu.lo;
        is_init = (r == 0);
        i = t_min - offs[r];
      }
      double prev = 0.0, e1 = 1.0, e2 = 1.0, e3 = 1.0;
      // path DP state of the row: running maximum of the previous row's scores (raw, as received,
      // and normalised by 2^rho), the row's accumulated exponent G (the tolerance margin is a function of the
      // two, formed only where a tie is near: path_step.h)
      double bestn = 0.0;
      // scale of bestn, and so of this row's scores.  Row 0 starts the scores at scale 0: its lane reads the zero entry
      // on every step (Lane3::pA), so nothing ever updates its maximum and G stays the 0 it hands on.
      int G = is_init ? 0 : GBIG;
      // Flush detector.  In a banded forward-backward pass every allowed path crosses every row
      // exactly once, so sum_i prefix[r][i] * suffix[r][i] is the SAME total for every row r.
      // Cells far below the wave's scale flush to zero here; if that ever removes mass that
      // matters, some row's sum deviates — checked over all rows at the end of the read.
      double rsum = 0.0, smin = INFINITY, smax = 0.0;
      uint32_t bits = 0;
      int r_old = min(64 * wv, T);  // the oldest open row of this wave
      // sample index of the oldest open row (scalar): t_min for row 0 (offs[0] = 0)
      int i_old = (r_old < T) ? __builtin_amdgcn_readfirstlane(i) : -0x40000000;
      int e_old = (r_old < T) ? __builtin_amdgcn_readfirstlane(be) : 0x40000000;  // (one wave per read) its band end
      int filled_hi = ((i_old - MEL - 1) > 0 ? (i_old - MEL - 1) / CH : 0) * CH;
      while (i_old + 2 >= filled_hi) {
        for (int w = lane; w < CH; w += 64) {
          int idx = filled_hi + w;
          ring[idx & RM] = (idx >= 0 && idx < N) ? sig[idx] : 0.0;
        }
        filled_hi += CH;
      }
      double nxt;  // the chunk above the filled ones, loaded one refill ahead (see the reverse sweep)
      {
        const int idx = filled_hi + lane;
        nxt = (idx >= 0 && idx < N) ? sig[idx] : 0.0;
      }
      __syncthreads();
      Scale sc{0, 0, 0};
      int sh_until = 0;  // (scalar) steps below this one still see values from before the last scale move
      const int ip0 = PAIR ? pair_swap(i) : 0;
      if (PAIR) {
        const double pmn = pair_swap(mean), pac = pair_swap(ac2), pmc = pair_swap(mc2);
        if (!em) { mean = pmn; ac2 = pac; mc2 = pmc; }
        // step 0 is even: the transition lane holds its partner's density of step 1, sample s[ip]
        ia = em ? i - 1 : ip0;
      } else {
        ia = i - 1;
      }
      double e = density(ring[ia & RM], mean, ac2, mc2, 0, etab);
      if (PAIR) ia = (em ? i : ip0 + 1) + 1;  // first evaluation at step 1
      int init_live = 1;  // (uniform, scalar registers) row 0 is still being swept
      int top_live = (top < TL) ? 1 : 0;  // the last row has been started

      // The prefetch ring: PF / 2 loads of 16 bytes in flight, PF steps ahead.  (The scheduler issues these first
      // loads last slot first, so on the way in cur_v[0] is the youngest and the wait at the head of a trip, which
      // has to hold on that way too, is for ALL loads in flight, vmcnt(0), where PF / 2 - 1 could stay out.  A
      // scheduling barrier behind each load here keeps them in step order and turns that wait into vmcnt(3) on
      // every even step — measured SLOWER, forward launch +0.7 %, and not kept: DESIGN.md 5.1a.)
      double2 cur_v[PF / 2];
#pragma unroll
      for (int q = 0; q < PF / 2; q++) cur_v[q] = spill_load2(spill_rs, lane16, q);
      // The reverse sweep's scale, one value per RS steps, comes through the scalar cache: it is
      // uniform, and a vector load per step would put one more operation on the wait counter that
      // guards the spill prefetch.  The cache was invalidated after the reverse sweep's stores.
      const __attribute__((address_space(4))) int32_t *sL =
          (const __attribute__((address_space(4))) int32_t *)(uintptr_t)spill_L;
      int Lrev = 0;

      // (16 steps per trip would make `age` a compile-time constant and most rare-path tests static;
      // measured: 18.7 instead of 17.6 ms — the loop no longer fits the instruction cache.  4 steps per
      // trip: 17.8 ms.)
      for (int ub = 0; ub < n_steps; ub += FT) {
#pragma unroll
        for (int q = 0; q < FT; q++) {
          const int u = ub + q;
          {  // (n_steps is a multiple of 32 = 4 trips: no end test inside a trip)
            const int age = u & (RS - 1);
            if (age == 0 && u > 0) {
              sc.L += sc.d_next;
              sc.d_last = sc.d_next;
              sh_until = (sc.d_next != 0) ? u + c + MEL : 0;
              sc.d_next = 0;
              if (PAIR) { cq = ldexp(cq, sc.d_last); dsel = 0; }
            }
            if (PAIR && age == 1 && u > 1) cq = ldexp(cq, -sc.d_last);
            shift_now = (age == 0 && u > 0) ? sc.d_last : 0;
            if constexpr (W == 1) {
              if (i_old > e_old) {  // see the reverse sweep
                int sw_em = 0;
                do {
                  const int fl = r_old & 63;
                  const int rn = r_old + 64;  // the row that lane takes
                  Lane3 nx = lane3_sload(fwdl + min(rn, top));
                  // (no row left for that lane: the clamped record made inert, see the reverse sweep)
                  const int nm = __builtin_amdgcn_readfirstlane(top - rn) >> 31;
                  nx.end = (nx.end & ~nm) | (0x40000000 & nm);
                  nx.pA = (nx.pA & ~nm) | (0x40000000 & nm);
                  nx.pW &= ~nm;
                  if (lane == fl) {
                    // (the verdict of path_step.h's bound on G travels with the row mass: a sum no row can have)
                    smin = fmin(smin, (abs(G) >= path_step::PATH_G_GUARD) ? -1.0 : rsum);
                    smax = fmax(smax, rsum);
                    rsum = 0.0;
                    r = rn;
                    prev = 0.0;
                    bestn = 0.0; G = GBIG;
                    i -= nx.mg >> 12;
                    TAKE_LANE(nx);
                    be = nx.end; lo = nx.lo;
                  }
                  if (PAIR) sw_em |= ~nm & fl;  // (bit 0: the forward sweep's emitting lanes are the odd ones)
                  r_old += 1;
                  const int io = __builtin_amdgcn_readlane(i, r_old & 63), eo = __builtin_amdgcn_readlane(be, r_old & 63);
                  i_old = (r_old < T) ? io : -0x40000000;
                  e_old = (r_old < T) ? eo : 0x40000000;
                } while (i_old > e_old);
                if (PAIR) {
                  if (sw_em & 1) {
                    const double pmn = pair_swap(mean), pac = pair_swap(ac2), pmc = pair_swap(mc2);
                    const int ip = pair_swap(i);
                    if (!em) { mean = pmn; ac2 = pac; mc2 = pmc; }
                    ia = (em ? i : ip + 1) + ((u & 1) ? 0 : 1);
                  }
                }
                // (from the row counter, as sign bits: r_old == 0; r_old <= top < r_old + 64)
                unsigned blk = (unsigned)(top - r_old) >> 6;
                blk = (unsigned)__builtin_amdgcn_readfirstlane((int)blk);
                init_live = (int)((unsigned)(r_old - 1) >> 31);
                top_live = (int)((blk - 1u) >> 31);
              }
            } else {
            bool fin = (i > be);
            if (__any(fin)) {
              bool redo = false;
              for (unsigned long long fm = __builtin_amdgcn_ballot_w64(fin); fm != 0; fm &= fm - 1) {
                const int fl = __builtin_ctzll(fm);
                const int rn = __builtin_amdgcn_readlane(r, fl) + TL;  // (uniform) the row that lane takes
                Lane3 nx;
                nx.mean = nx.ac = nx.mc = 0.0; nx.bs = nx.end = nx.lo = nx.pA = nx.pW = nx.mg = 0;
                if (rn < T) nx = lane3_sload(fwdl + rn);
                if (lane == fl) {
                  smin = fmin(smin, rsum);
                  smax = fmax(smax, rsum);
                  rsum = 0.0;
                  r = rn;
                  i -= nx.mg >> 12;
                  prev = 0.0;
                  suspect |= (abs(G) >= path_step::PATH_G_GUARD);  // path_step.h: the margin-free comparison's bound
                  bestn = 0.0; G = GBIG;
                  if (r < T) {
                    TAKE_LANE(nx);
                    be = nx.end; lo = nx.lo;
                    is_init = false;
                    redo = true;
                  } else {
                    lo = 0x40000000; be = 0x40000000; pA = 0x40000000; pW = 0;
                    if (PAIR && !em) cq = 0.0;
                  }
                }
              }
              if (PAIR) {  // see the reverse sweep
                if (__any(redo && em)) {
                  const double pmn = pair_swap(mean), pac = pair_swap(ac2), pmc = pair_swap(mc2);
                  const int ip = pair_swap(i);
                  if (!em) { mean = pmn; ac2 = pac; mc2 = pmc; }
                  const int odd = u & 1;
                  if (W > 1) {  // (see the reverse sweep)
                    redo = em ? redo : !odd;
                    if (redo) e = density(ring[(em ? i - 1 : ip) & RM], mean, ac2, mc2, em ? shift_now : 0, etab);
                  }
                  ia = (em ? i : ip + 1) + (odd ? 0 : 1);
                }
              } else if (W > 1 && redo) {
                e = density(ring[(i - 1) & RM], mean, ac2, mc2, shift_now, etab);
              }
              while (r_old < T && __builtin_amdgcn_readlane(r, r_old & 63) != r_old)
                r_old += (W > 1 && (r_old & 63) == 63) ? 1 + 64 * (W - 1) : 1;  // (the wave's rows only)
              // (no open row left: a sample index no refill test ever reaches)
              i_old = (r_old < T) ? __builtin_amdgcn_readlane(i, r_old & 63) : -0x40000000;
              init_live &= (__builtin_amdgcn_readfirstlane(r) == 0) ? 1 : 0;
              top_live = (__builtin_amdgcn_readlane(r, top & 63) == top) ? 1 : 0;
            }
            }
            {
              const int need_max = i_old + (PAIR ? 2 : 1);  // (PAIR: the partner evaluates one sample further ahead)
              while (need_max >= filled_hi) {
                RING_SYNC();
                ring[(filled_hi + lane) & RM] = nxt;
                filled_hi += CH;
                {
                  const int idx = filled_hi + lane;
                  nxt = (idx >= 0 && idx < N) ? sig[idx] : 0.0;
                }
                RING_SYNC();
              }
            }
            // LDS reads first: the neighbour's values and the sample of the next step's density
            const int hs = ((unsigned)(i - pA) <= (unsigned)pW) ? ra : HZv;  // else: the zero entry
            const bool evalstep = !PAIR || (q & 1);  // (static) PAIR: densities are evaluated on odd steps
            double xn = 0.0;
            if (evalstep) xn = ring[(PAIR ? ia : i) & RM];
            const double2 hv = hist2[hs];
            const int Gin = ghist[hs];
            const bool sh_any = (u < sh_until);
            DensHalf dn;
            if (evalstep) dn = density_begin(xn, mean, ac2, mc2, etab);
            // ---- the cell (r, i): out = P * pred[i - mel] + e(s[i-1]) * out[i - 1]
            // (the band test is only needed on the rare paths below: outside the band the posterior is zero
            // by itself, see `post`, and outside the lane's span its value is, see Lane3::pA)
#define IN_BAND ((i >= lo) && (i <= be) && (i >= bs))
            double P = emission_product<MEL>(e, e1, e2, e3);
            if (MEL > 0) P = fma(P, pm, qm);
            const double pv = hv.x, dv = hv.y;
            double t1 = P * pv;
            if (sh_any) {  // see the reverse sweep
              asm volatile("");
              t1 = ldexp(t1, ((age < D) ? sc.d_last : 0) - ((age < melr) ? sc.d_last : 0));
            }
            const double ee = PAIR ? fma(e, pm, cq) : e;
            double o = fma(ee, prev, t1);
            // (row 0's cells are set, not computed: with the other rare case, the last row's arg-max, below)
            // ---- posterior of the cell, on the scale 2^-K:  post = prefix * suffix
            const double suf = (q & 1) ? cur_v[(q % PF) >> 1].y : cur_v[(q % PF) >> 1].x;
            const int ur = n_steps - 1 - u;  // the reverse sweep's step for this anti-diagonal
            // (the period divides n_steps: the reverse sweep's rescale steps are this sweep's age-0 steps)
            if (age == 0) Lrev = sL[ur >> RSH];
            const int kap = -(sc.L + K) - Lrev;  // scalar
            // No band test here: a cell of the lane's warm-up (lo <= i < bs) has suf == 0, because the
            // reverse sweep's lane was idle at this (step, lane) — it leaves row r at bs and the planner
            // keeps its next row (r - 64) from reaching back into [lo, be] of row r — and beyond `be`
            // o is 0.  (A violation would show up in the row-mass check.)
            double post = ldexp(o * suf, kap);
            // ---- path step (node.cpp:52-91): running maximum of the previous row, strict '>' at the
            // resolution of the reference's log-doubles (xm::gt_tol): margin = best * |exponent| * 2^-52
            // Scores are (double, integer scale): stored = true * 2^scale.  The running maximum is kept
            // normalised (bestn in [0.5,1), scale G); an incoming score is brought onto that scale
            // before comparing (far below -> 0, far above -> inf, both compare correctly).
            // The margin is formed only where some lane's pair is inside the tie margin: everywhere else
            // tdiff > margin and tdiff > 0 are the same bit (path_step.h has the lemma and its bound on G).
            const double dva = ldexp(dv, G - Gin);  // no maximum yet: G = GBIG, any dv > 0 becomes +inf
            const double tdiff = dva - bestn;
            bool upd = (tdiff > 0.0);  // (dv == 0 outside the span: never an update)
            // The tie flag (include/nadavca_hip.h, parity contract): the two scores are closer than 2^-24
            // relative — far more than the rounding either this engine or the reference accumulates, so a
            // read without the flag has the reference's decisions everywhere.  (A candidate of 0, or the
            // +inf a first candidate turns into, never qualifies.  Scores of cells thousands of bits below
            // the path would tie by their lost precision: this file is compiled with FP64 denormals
            // flushed, which makes them exact zeros.)
            {
              const unsigned long long nr = __builtin_amdgcn_ballot_w64(path_step::path_near(tdiff, dva));
              if (nr != 0) {  // (rare, a scalar branch: the margin and the classes are sorted out off the usual path)
                asm volatile("");
                const double bthr = path_step::path_margin(bestn, G);
                // (through a ballot: as a second compare of tdiff the compiler merges it with the usual path's and
                // carries the margin, a zero there, in two registers again)
                upd = ((__builtin_amdgcn_ballot_w64(tdiff > bthr) >> lane) & 1) != 0;
                const unsigned long long zr = __builtin_amdgcn_ballot_w64(path_step::path_tie_exact(tdiff));
                const unsigned long long ur = __builtin_amdgcn_ballot_w64(path_step::path_tie_ulp(tdiff, bthr));
                amb_x |= nr & zr;
                amb_u |= nr & ur & ~zr;
                amb_n |= nr & ~ur & ~zr;
              }
            }
            if (upd) {
              asm volatile("");  // (keeps the three instructions under the lane mask: as selects they are six)
              path_step::path_take(dv, Gin, bestn, G);  // bestn in [0.5, 1), G its scale; -G = true exponent
            }
            bits = (bits << 1) | (upd ? 1u : 0u);  // step u ends up at bit 31 - (u & 31)
            double dpv = bestn * post;  // post is already 0 outside the band
            if (init_live | top_live) {  // (one scalar test for the two rare cases: the first and the last row)
              asm volatile("");
              if (init_live) {
                if ((W == 1) ? (r == 0) : is_init) {  // (see the reverse sweep)
                  o = IN_BAND ? ldexp(1.0, sc.L) : 0.0;
                  post = ldexp(o * suf, kap);
                  dpv = post;  // (on scale G = 0, see above)
                }
              }
              if (top_live) {
              const double da = ldexp(dpv, (fbest == 0.0) ? 0 : fG - G);
              const double fdiff = da - fbest;
              bool fupd = (fdiff > 0.0);  // (as above: the margin only where a tie is near)
              {
                const unsigned long long nr = __builtin_amdgcn_ballot_w64(r == top && IN_BAND && path_step::path_near(fdiff, da));
                if (nr != 0) {
                  asm volatile("");
                  const double fthr = path_step::path_top_margin(fbest, fG);
                  fupd = (fdiff > fthr);
                  const unsigned long long zr = __builtin_amdgcn_ballot_w64(path_step::path_tie_exact(fdiff));
                  const unsigned long long ur = __builtin_amdgcn_ballot_w64(path_step::path_tie_ulp(fdiff, fthr));
                  amb_x |= nr & zr;
                  amb_u |= nr & ur & ~zr;
                  amb_n |= nr & ~ur & ~zr;
                }
              }
              if (r == top && IN_BAND && fupd) {
                fbest = dpv;
                fG = G;
                fidx = i;
              }
              }
            }
            prev = o;
            rsum += post;
            *reinterpret_cast<double2 *>(histb + (su * (16 * TL) + gl16)) = make_double2(o, dpv);
            *reinterpret_cast<int *>(ghistb + (su * (4 * TL) + (gl16 >> 2))) = G;
            if ((u & 31) == 31) {
              int w = u >> 5;
              asm volatile("" : "+s"(w));  // keeps the address arithmetic inside the branch
              bp[(size_t)w * TL + gl] = bits << (31 - (u & 31));
              bits = 0;
            }
            // refill the prefetch slot just consumed
            if (q & 1) cur_v[(q % PF) >> 1] = spill_load2(spill_rs, lane16, (u + PF) >> 1);
            // ---- rescale decision for the next step, then the next step's density
            if (W > 1 && age == RS - 2) {  // see the reverse sweep
              const int mxw = wave_max_i((o != 0.0) ? __builtin_amdgcn_frexp_exp(o) : -0x40000000);
              if (lane == 0) tmax[wv] = mxw;
            }
            if (age == RS - 1) {
              suspect |= !(o <= HUGE_V);
              if (W == 1) suspect |= (i > be);  // (the switch order's guard, see the reverse sweep)
              int mx;
              if (W == 1) {
                mx = wave_max_i((o != 0.0) ? __builtin_amdgcn_frexp_exp(o) : -0x40000000);
              } else {
                mx = tmax[0];
#pragma unroll
                for (int w = 1; w < W; w++) mx = max(mx, tmax[w]);
                mx = __builtin_amdgcn_readfirstlane(mx);
              }
              sc.d_next = (mx > -0x40000000) ? min(TARGET - mx, DMAX) : 0;
              suspect |= (u + 1 < n_steps) && (mx > -0x40000000) && (TARGET - mx > DMAX);
              if (PAIR) dsel = em ? sc.d_next : 0;
            }
            i += 1;
            i_old += 1;
            e3 = e2; e2 = e1; e1 = e;
            if (!PAIR) {
              e = density_end(dn, sc.d_next);
            } else if (evalstep) {
              e = density_end(dn, dsel);
              ia += 2;
            } else {
              e = pair_swap(e);
            }
            su = (su + 1 == H) ? 0 : su + 1;
            ra = (int)min((unsigned)(ra + TL), (unsigned)(ra + TL - HZ));
            STEP_SYNC();
          }
        }
      }
      if (r < T) {  // rows still open when the sweep ends
        smin = fmin(smin, rsum);
        smax = fmax(smax, rsum);
        suspect |= (abs(G) >= path_step::PATH_G_GUARD);
      }
      for (int dlt = 32; dlt >= 1; dlt >>= 1) {
        smin = fmin(smin, __shfl_xor(smin, dlt, 64));
        smax = fmax(smax, __shfl_xor(smax, dlt, 64));
      }
      suspect |= !(smin > 0.0 && smax <= smin * (1.0 + MASS_TOL));
    }
    __syncthreads();

    // ====================================== traceback ============================================
    int idx = __shfl(fidx, top & 63, 64);
    bool any_suspect = __any(suspect);
    if (W > 1) {  // the team's verdict: any wave's range guard or tie flag, the arg-max of the wave that held `top`
      if (lane == 0) tflag[wv] = (any_suspect ? 1 : 0) | (amb_x != 0 ? 2 : 0) | (amb_n != 0 ? 4 : 0) | (amb_u != 0 ? 8 : 0);
      if (gl == (top & (TL - 1))) *tfidx = fidx;
      __syncthreads();
      int fl = 0;
#pragma unroll
      for (int w = 0; w < W; w++) fl |= tflag[w];
      any_suspect = (fl & 1) != 0;
      amb_x = (fl & 2) ? 1ull : 0ull;
      amb_n = (fl & 4) ? 1ull : 0ull;
      amb_u = (fl & 8) ? 1ull : 0ull;
      idx = *tfidx;
    }
    if (any_suspect || (idx < 0 && K != 0)) {
      // out of range somewhere, or no path although the suffix sweep found mass: exact kernel
      if (gl == 0) {
        g.out_status[rd] = NVK_READ_RETRY_INTERNAL;
        atomicAdd(g.n_retry, 1);
      }
      continue;
    }
    if (idx < 0) {
      if (gl == 0) g.out_status[rd] = NVK_READ_NO_PATH;
      continue;
    }
    if (gl == 0 && ((amb_x | amb_n | amb_u) != 0 || m.rsv))
      g.ties[rd] = (amb_x != 0 ? NVK_TIE_EXACT : 0) | (amb_n != 0 ? NVK_TIE_NEAR : 0) | (amb_u != 0 ? NVK_TIE_ULP : 0) |
                   (m.rsv ? NVK_TIE_PLATEAU : 0);
    if (wv == 0) {  // (of a team, its first wave)
      // The walk down the update bits: row r's word tells where row r - 1 starts, a serial chain of ~800 rows per
      // read.  Run by one lane it was ~60 instructions per row — 9 % of everything the wave issues, and a wave that
      // shares its SIMD with three sweeping ones gets an issue slot every ~16 cycles whatever the instruction is.
      // Here the wave prepares 16 rows at a time in its lanes (lane 4 l + q: row r0 - l, its offsets folded into
      // two constants, and the q-th of four consecutive bit words around the step a straight line through the read
      // predicts), and the serial part is scalar: three v_readlane, a handful of SALU operations, one v_writelane
      // for the event boundary, which the lanes store together after the 16 rows.  A word outside the four, or an
      // empty one, goes the old way.  Same bits, same arithmetic, same result.
      int32_t *ev = g.out_events + 2 * m.ref_off;
      const float steps_per_row = (float)n_steps / (float)T;
      int st = NVK_READ_OK;
      int r = top;
      int cur = __builtin_amdgcn_readfirstlane(idx);  // the chain below is scalar: every value of it in SGPRs
      while (r >= 0) {
        const int r0 = r;
        const int l = lane >> 2, q = lane & 3;
        const int row = r0 - l;
        const int off_l = (row >= 0) ? offs[row] : 0;
        const int pm_l = g.transitions ? ((row - 1) & 1 ? 0 : MEL) : MEL;
        const int a_l = off_l - t_min;            // u = cur + a
        const int b_l = t_min - off_l - pm_l;     // next cur = (step of the bit) + b
        const int u0 = cur + __builtin_amdgcn_readfirstlane(a_l);
        const int wq = ((u0 - (int)((float)l * steps_per_row)) >> 5) + 1 - q;
        const uint32_t word = (row >= 1 && wq >= 0) ? bp[(size_t)wq * TL + (row & (TL - 1))] : 0u;
        int curs = cur;  // lane ll: the event boundary of row r0 - ll
        int done = 0;
        for (int ll = 0; ll < 16; ++ll) {
          curs = (lane == ll) ? cur : curs;
          done = ll + 1;
          if (r == 0) {
            r = -1;
            break;
          }
          const int u = cur + __builtin_amdgcn_readlane(a_l, 4 * ll);
          int w = u >> 5;
          const int qi = __builtin_amdgcn_readlane(wq, 4 * ll) - w;  // lane 4 ll holds the highest of the four words
          uint32_t v = 0;
          if ((unsigned)qi <= 3u)
            v = (uint32_t)__builtin_amdgcn_readlane((int)word, 4 * ll + qi) & (0xffffffffu << (31 - (u & 31)));
          if (v == 0) {  // not among the four, or no bit at or below u in that word: the plain walk for this row
            v = (uint32_t)__builtin_amdgcn_readfirstlane((int)bp[(size_t)w * TL + (r & (TL - 1))]) &
                (0xffffffffu << (31 - (u & 31)));
            while (v == 0 && w > 0) {
              --w;
              v = (uint32_t)__builtin_amdgcn_readfirstlane((int)bp[(size_t)w * TL + (r & (TL - 1))]);
            }
            if (v == 0) {
              st = NVK_READ_RETRY_INTERNAL;
              if (lane == 0) atomicAdd(g.n_retry, 1);
              r = -1;
              break;
            }
          }
          cur = (w << 5) + (31 - (__ffs(v) - 1)) + __builtin_amdgcn_readlane(b_l, 4 * ll);
          --r;
        }
        // the boundaries of rows r0 .. r0 - done + 1, stored by as many lanes
        if (lane < done) {
          const int rr = r0 - lane;
          if (g.transitions) {
            ev[2 * (rr >> 1) + (rr & 1)] = curs;
          } else {
            if (rr > 0) ev[2 * (rr - 1) + 1] = curs;
            if (rr < top) ev[2 * rr] = curs;
          }
        }
      }
      if (lane == 0) g.out_status[rd] = st;
    }  // (a team's other waves have nothing to do here)
  }
}

typedef void (*Align3Kernel)(Align3Args);

template <int MEL, int RSH, bool PAIR, int W>
bool set_sweeps(Align3Kernel k[2]) {  // [0] reverse sweeps, [1] forward sweeps
  k[0] = align3_kernel<MEL, RSH, PAIR, 1, W>;
  k[1] = align3_kernel<MEL, RSH, PAIR, 2, W>;
  return true;
}

// The kernels that are built: one wave per read keeps the base period (see launch_align3), a team takes the
// period its skew needs.  PAIR (transition rows): the paired variant.  false: no kernel for this combination.
template <int MEL>
bool sweeps_of(bool pair, int W, int rsh, Align3Kernel k[2]) {
  constexpr int TW = ALIGN3_TEAM_W;
  if (W == 1) {
    if (pair && rsh == 4) return set_sweeps<MEL, 4, true, 1>(k);
    if (!pair && rsh == 3) return set_sweeps<MEL, 3, false, 1>(k);
    return false;
  }
  if (W != TW) return false;
  switch (rsh) {
    case 3: return !pair && set_sweeps<MEL, 3, false, TW>(k);
    case 4: return pair ? set_sweeps<MEL, 4, true, TW>(k) : set_sweeps<MEL, 4, false, TW>(k);
    case 5: return pair ? set_sweeps<MEL, 5, true, TW>(k) : set_sweeps<MEL, 5, false, TW>(k);
    default: return false;
  }
}

bool select_sweeps(int mel, bool pair, int W, int rsh, Align3Kernel k[2]) {
  switch (mel) {
    case 0: return sweeps_of<0>(pair, W, rsh, k);
    case 1: return sweeps_of<1>(pair, W, rsh, k);
    case 2: return sweeps_of<2>(pair, W, rsh, k);
    case 3: return sweeps_of<3>(pair, W, rsh, k);
    case 4: return sweeps_of<4>(pair, W, rsh, k);
    default: return false;
  }
}

}  // namespace

// What select_sweeps builds, asked of select_sweeps itself (include/nadavca_hip.h): every argument over a range wider
// than any launcher passes.
extern "C" int nvk_built_sweep_variants(int cap, int32_t *out, int *n_variants) {
  if (cap < 0 || (cap > 0 && !out) || !n_variants) return NVK_ERR_INVALID;
  int n = 0;
  Align3Kernel k[2];
  for (int mel = 0; mel < 8; mel++)
    for (int pair = 0; pair < 2; pair++)
      for (int W = 1; W <= 8; W++)
        for (int rsh = 0; rsh <= 8; rsh++) {
          if (!select_sweeps(mel, pair != 0, W, rsh, k)) continue;
          if (n < cap) {
            out[4 * n] = mel;
            out[4 * n + 1] = pair;
            out[4 * n + 2] = W;
            out[4 * n + 3] = 1 << rsh;
          }
          ++n;
        }
  *n_variants = n;
  return NVK_OK;
}

// One work counter per sweep launch, so that nothing has to be zeroed between a chunk's reverse and forward
// launch: the first 64 bytes of WS_MISC are 16 counters, zeroed together up front (align3_prepare) and again (in
// stream order, before a reverse launch) whenever a batch of many chunks has used them all.
constexpr int N_COUNTERS = 16;
static_assert(N_COUNTERS % 2 == 0, "a chunk's reverse / forward pair of counters must not straddle a re-zero");

int align3_reserve(nvk_ctx *ctx, int64_t n_reads) {
  int rc = nvk_ws_reserve(ctx, WS_MISC, 256);
  if (rc) return rc;
  return nvk_ws_reserve(ctx, WS_RSTATE, (size_t)n_reads * sizeof(int2));
}

int align3_prepare(nvk_ctx *ctx, int64_t *spill_cap) {
  NVK_HIP(hipMemsetAsync(ctx->ws[WS_MISC], 0, N_COUNTERS * sizeof(int), ctx->stream));
  *spill_cap = nvk_spill_cap(ctx, WS_SPILL);
  return NVK_OK;
}

int launch_align3(nvk_ctx *ctx, const BatchArgs &a, int transitions, const ReadMeta *metas, const PlanTotals &tot,
                  const int *order, const int32_t *steps_sorted, int32_t *out_events, int32_t *out_status,
                  int *d_retry, int64_t spill_cap) {
  static_assert(WS_OFFS < (int)(sizeof(ctx->ws) / sizeof(ctx->ws[0])), "workspace table too small");
  if (a.n_reads == 0) return NVK_OK;
  const int mel = a.mel;
  if (mel < 0 || mel > 4) {
    nvk_set_error("min_event_length %d outside the compiled range 0..4", mel);
    return NVK_ERR_UNSUPPORTED;
  }
  const int max_c = tot.max_c < 1 ? 1 : tot.max_c;
  int *counter = (int *)ctx->ws[WS_MISC];
  int launches = 0;

  // Two launches: the LDS rings are sized by the largest skew a launch serves, so the (usual) reads
  // with c <= ALIGN1_C_CAP keep their 16 waves per CU whatever else is in the batch; wide-band reads
  // (long reads, BASELINE config 5) run with larger rings and a longer rescale period.
  // (wide bands: teams of ALIGN3_TEAM_W waves, ReadMeta::cw; their history ring of (cw + mel + 1) slots of
  // 256 lanes x 20 B has to fit the 160 KB of a CU)
  constexpr int C_HARD = 24;
  // (mel <= 4: one wave per read keeps the base period of 8 or 16 steps, a team's stays within 32 — rsh below)
  static_assert(ALIGN1_C_CAP + 4 < 8 && C_HARD + 4 < 32, "no kernel for the rescale period these skews need");
  struct Cls { int hi; int W; };
  Cls cls[2];
  int ncls = 0;
  const int64_t n_wide = (int64_t)tot.n_wide;
  const int max_cw = tot.max_cw < 1 ? 1 : tot.max_cw;
  if (a.n_reads - n_wide > 0 || max_c <= ALIGN1_C_CAP)
    cls[ncls++] = Cls{max_c < ALIGN1_C_CAP ? max_c : ALIGN1_C_CAP, 1};
  if (max_c > ALIGN1_C_CAP) cls[ncls++] = Cls{max_cw < C_HARD ? max_cw : C_HARD, ALIGN3_TEAM_W};
  int rc = NVK_OK;
  TimerScope ts_align(ctx, NVK_K_ALIGN);
  for (int k = 0; k < ncls; k++) {
    int c = cls[k].hi;
    const int W = cls[k].W, TLk = 64 * W;
    // the widest skew whose rings fit a CU's LDS (reads beyond it go to the exact kernel)
    auto lds_need = [&](int cc, int slot_bytes) {
      const int Hc = (cc + mel > 0 ? cc + mel : 1) + (W > 1 ? 1 : 0);
      int SRc = 256;
      while (SRc < 64 * cc + CH) SRc <<= 1;
      return (size_t)ETN * 8 + (size_t)W * SRc * 8 + (size_t)Hc * TLk * slot_bytes + slot_bytes + 16 + 12 * W;
    };
    while (c > 1 && lds_need(c, 20) > 160 * 1024) --c;
    // Rescale period 16, or 8 without transition rows: there the last rows of a sweep run through
    // far-off-path cells with nothing slower beside them (the constant-density rows), the wave's
    // largest value collapses ~70 bits per step, and a period of 16 steps overruns the scale-move cap
    // on 1-2 % of the reads (each such read costs a pass of the exact kernel).
    int rsh = transitions ? 4 : 3;
    // (a neighbour value is at most c + mel steps old: a period of c + mel + 1 steps already keeps two
    // rescale steps out of its way)
    while ((1 << rsh) <= c + mel) rsh++;
    Align3Kernel kern[2];
    if (!select_sweeps(mel, transitions != 0, W, rsh, kern)) {
      nvk_set_error("no align3 kernel for min_event_length %d, transitions %d, %d waves, rescale period %d", mel,
                    transitions, W, 1 << rsh);
      return NVK_ERR_UNSUPPORTED;
    }
    // history ring: ages 1 .. c+mel are read; the oldest slot is read and then overwritten in the
    // same step (LDS operations of one wave execute in program order)
    // (a team's ring has one slot more: across waves "read the oldest slot, then overwrite it" is a race)
    const int H = (c + mel > 0 ? c + mel : 1) + (W > 1 ? 1 : 0);
    int SR = 256;
    while (SR < 64 * c + CH) SR <<= 1;  // per wave
    // exp table + the waves' signal rings + history ring (+ its zero entry) + work item / team exchange words
    const size_t lds = lds_need(c, 20);
    const size_t lds_rev = lds_need(c, 8);  // reverse-only launch
    if (lds > 160 * 1024) return NVK_ERR_UNSUPPORTED;
    int per_cu = (int)((160 * 1024) / lds);          // workgroups (waves, or teams of W waves) per CU
    if (per_cu > 4 * LB / W) per_cu = 4 * LB / W;
    if (per_cu < 1) per_cu = 1;
    int per_cu_rev = (int)((160 * 1024) / lds_rev);
    if (per_cu_rev > 4 * (W > 1 ? LB_REV_TEAM : LB_REV) / W) per_cu_rev = 4 * (W > 1 ? LB_REV_TEAM : LB_REV) / W;
    if (per_cu_rev < 1) per_cu_rev = 1;
    int32_t mxpad = 1;  // the longest read of the batch under the offsets the kernels use (ReadMeta::pad)
    for (int64_t q = 0; q < a.n_reads; q++) mxpad = steps_sorted[q] > mxpad ? steps_sorted[q] : mxpad;
    const int64_t bp_stride = (int64_t)((mxpad + 31) / 32 + 1) * TLk;
    // (the second class asks again: the first one's chunks may have grown the workspaces)
    const int64_t cap = (k == 0) ? spill_cap : nvk_spill_cap(ctx, WS_SPILL);

    Align3Args g;
    g.metas = metas;
    g.fwdl = (const Lane3 *)ctx->ws[WS_LANE_F];
    g.revl = (const Lane3 *)ctx->ws[WS_LANE_R];
    g.offs = (const int32_t *)ctx->ws[WS_OFFS];
    g.signal = a.signal;
    g.bp_stride = bp_stride;
    g.order = order;
    g.H = H;
    g.SR = SR;
    g.transitions = transitions;
    g.c_cap = c;
    g.flag_above = (k == ncls - 1) ? 1 : 0;
    g.rstate = (int2 *)ctx->ws[WS_RSTATE];
    g.n_retry = d_retry;
    g.ties = (int32_t *)ctx->ws[WS_TIES];
    g.out_events = out_events;
    g.out_status = out_status;
    for (int ph = 0; ph < 2; ph++)
      if ((ph == 0 ? lds_rev : lds) > 64 * 1024)
        NVK_HIP(hipFuncSetAttribute((const void *)kern[ph], hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(ph == 0 ? lds_rev : lds)));
    // chunks of launch positions whose spill fits the cap; a chunk's slots are sized by its longest read.
    // The launch order is class-major (launch_order): the teams' reads are positions [0, n_wide), the one-wave
    // reads the rest, so a class's chunks, slots and workgroups count only the reads it sweeps.
    const int64_t pos_lo = (W > 1) ? 0 : n_wide, pos_hi = (W > 1) ? n_wide : a.n_reads;
    int64_t lo = pos_lo;
    int64_t n_chunks = 0;
    while (lo < pos_hi) {
      int64_t hi = lo, mx = 1;
      while (hi < pos_hi) {
        const int64_t m2 = steps_sorted[hi] > mx ? steps_sorted[hi] : mx;
        if (hi > lo && (m2 + 2 * PF) * 512 * W * (hi - lo + 1) > cap) break;
        mx = m2;
        ++hi;
      }
      int64_t n_chunk = hi - lo;
      int64_t spill_stride = (mx + 2 * PF) * 64;
      // (the cap is an estimate of what is free: if the allocation still fails, serve half as many reads)
      while ((rc = nvk_ws_reserve(ctx, WS_SPILL, (size_t)n_chunk * W * spill_stride * 8)) == NVK_ERR_NOMEM &&
             n_chunk > 1) {
        n_chunk = (n_chunk + 1) / 2;
        hi = lo + n_chunk;
        mx = 1;
        for (int64_t q = lo; q < hi; q++) mx = steps_sorted[q] > mx ? steps_sorted[q] : mx;
        spill_stride = (mx + 2 * PF) * 64;
      }
      if (rc) return rc;
      const int64_t L_stride = (mx >> rsh) + 4;
      rc = nvk_ws_reserve(ctx, WS_STAGE, (size_t)n_chunk * L_stride * 4);
      if (rc) return rc;
      int64_t slots_f = ctx->slots_override > 0 ? ctx->slots_override : (int64_t)ctx->num_cus * per_cu;
      int64_t slots_r = ctx->slots_override > 0 ? ctx->slots_override : (int64_t)ctx->num_cus * per_cu_rev;
      if (slots_f > n_chunk) slots_f = n_chunk;
      if (slots_r > n_chunk) slots_r = n_chunk;
      rc = nvk_ws_reserve(ctx, WS_BP, (size_t)slots_f * bp_stride * 4);
      if (rc) return rc;
      g.spill_v = (double *)ctx->ws[WS_SPILL];
      g.spill_L = (int32_t *)ctx->ws[WS_STAGE];
      g.bp = (uint32_t *)ctx->ws[WS_BP];
      g.spill_stride = spill_stride;
      g.L_stride = L_stride;
      g.n_reads = (int)n_chunk;
      g.read_lo = (int)lo;
      if (launches > 0 && launches % N_COUNTERS == 0)
        NVK_HIP(hipMemsetAsync(counter, 0, N_COUNTERS * sizeof(int), ctx->stream));
      g.counter = counter + launches % N_COUNTERS;
      hipLaunchKernelGGL(kern[0], dim3((unsigned)slots_r), dim3(TLk), lds_rev, ctx->stream, g);
      g.counter = counter + (launches + 1) % N_COUNTERS;
      hipLaunchKernelGGL(kern[1], dim3((unsigned)slots_f), dim3(TLk), lds, ctx->stream, g);
      launches += 2;
      NVK_HIP(hipGetLastError());
      lo = hi;
      ++n_chunks;
    }
    // launch report (include/nadavca_hip.h): one record per class
    nvk_launch_note(ctx, nvk_launch_rec{NVK_LAUNCH_SWEEP, mel, transitions, W, 1 << rsh, 0, c, H, SR, (int32_t)lds,
                                        pos_hi - pos_lo, n_chunks});
  }
  // bytes the sweeps stream through HBM: 8 B written + 8 B read per (step, lane) + scales + bits
  ctx->last_spill_bytes = (int64_t)tot.steps * 64 * 16 + (int64_t)tot.steps / 16 * 8 + (int64_t)tot.steps * 8 * 2;
  return NVK_OK;
}
