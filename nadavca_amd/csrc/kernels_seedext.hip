// Extension stage of the seed aligner (nadavca_amd/seedalign.py): per read, a banded affine-gap local alignment
// against one strand of the reference around the diagonal its seeds voted for, then the traceback and the matched
// (read base, reference base) pairs.  The rules are those of include/nadavca_hip.h (nvk_seed_extend_dev); the CPU
// restatement the tests hold this kernel to is tests/host_shims/seedext_host.cpp.
//
// One wave64 per read; a persistent grid takes reads from an atomic counter.  The band is walked in strips of 64
// rows: lane l owns row i = 64 s + l of strip s and at step t computes the cell at band offset b = t - 2 l
// (b = j - i - (d* - w), 0 <= b <= 2w).  With that skew the up neighbour (i-1, b+1) is what lane l-1 computed one
// step earlier and the diagonal one (i-1, b) what it computed the step before that, so both arrive by a DPP
// rotate of the previous step's H and F; lane 0 takes them from the last row of the previous strip, which lane 63
// leaves in LDS.  The strip's reference window is staged in LDS once, already on the read's strand.
//
// Every cell's traceback nibble (2 bits of source, the E- and F-extend bits) goes to a device store, eight cells of
// a row to a dword, laid out [strip][dword column][lane] so that the 64 lanes' dwords of one column share lines.
// Lane 0 then walks the traceback; the pairs are written backwards from the read's last slot and the wave moves
// them down to start at q_off[j].  Nothing here depends on which reads share a launch, so the host may cut a batch
// into chunks when the store does not fit (nvk_seed_extend_dev).
//
// nvk_seed_extend_bounded_dev runs the same kernel with a reference range [ref_lo, ref_hi) per read, in coordinates of
// the read's strand (a contig of a multi-contig reference, nadavca_amd/refset.py): the two bounds are scalars of the
// wave like the read itself, and the sweep counts its columns from ref_lo, so its inner loop is the same for both
// entries.  The one kernel body is compiled twice (seedext_kernel<BOUNDED>): without bounds it is, instruction for
// instruction, the kernel it was before there were any.
//
// nvk_seed_extend_path_dev (seedext_kernel<BOUNDED, true>) lets the band follow a path: strip s of a read has its own
// centre, strip_diag[strip_off[j] + s] (from the seed chain, kernels_seedchain.hip), so the band's first diagonal lo
// is a scalar per strip instead of per read.  Inside a strip nothing changes.  At a strip's first row lane 0 finds
// its up and diagonal neighbours in the previous strip's last row at band offsets moved by delta = lo_s - lo_(s-1);
// an offset outside 0 .. 2w is no cell (H 0, F NEG: the slot behind the row's last).  Lane 63 writes that row while
// lane 0 still reads the previous one, which one buffer allows only for delta >= -127, so the path form keeps two
// and alternates.  The traceback takes lo from the strip of the row it stands on.  A centre so far off that its strip
// has no cell is pulled in to the nearest centre that still has none (path_lo): every diagonal then fits an int32.
// With PATH false the body is the one above, and the two kernels compiled from it are unchanged.
#include <vector>

#include "nvk_internal.h"
#include "part_cut.h"
#include "wave.h"

namespace {

constexpr int SEED_WMAX = 256;       // largest band half-width w compiled in
constexpr int SEED_NEG = -(1 << 30);
constexpr int SEED_MAX_READ = 1 << 26;   // keeps match * read length inside int32
constexpr int SEED_MAX_REF = 1 << 30;

struct SeedArgs {
  const int32_t *query;
  const int64_t *q_off;
  const int32_t *reference;  // forward strand
  int G;
  const int32_t *strand;
  const int32_t *diag;
  int w, match, mismatch, gap_open, gap_extend, min_score;
  int32_t *out_hit;          // 4 per read: score, end i, end j, pair count
  int2 *out_pairs;           // (i, j)
  uint32_t *tb;              // the traceback store less the chunk's first read's tb_off: read j's part is tb + tb_off[j]
  const int64_t *tb_off;     // per read, its first dword in the batch-wide numbering
  int r0, r1;                // the chunk's reads
  int *counter;
  const int32_t *ref_lo, *ref_hi;  // seedext_kernel<true>: per read, the range of its cells' j on its strand
  const int32_t *strip_diag;       // seedext_kernel<., true>: the band centre per strip of 64 rows, read j's strips
  const int64_t *strip_off;        // at strip_off[j] (diag is not read)
};

// a base code outside 0..3 never equals anything: -2 in the read, -1 in the reference
__device__ __forceinline__ int query_code(const int32_t *q, int64_t x) {
  const int c = q[x];
  return c >= 0 && c <= 3 ? c : -2;
}
__device__ __forceinline__ int ref_code(const int32_t *ref, int G, int st, int j) {
  if (j < 0 || j >= G) return -1;
  const int c = ref[st ? G - 1 - j : j];
  return c >= 0 && c <= 3 ? (st ? 3 - c : c) : -1;
}

// The first diagonal of a strip's band whose centre is d, for a read of m rows over the columns [rlo, rlo + Gr):
// d - w, with d held to rlo - m - w .. rlo + Gr + w.  Row i has cells iff d - w <= rlo + Gr - 1 - i and
// d + w >= rlo - i, so at either limit, as beyond it, no row 0 .. m - 1 has any.
__device__ __forceinline__ int path_lo(int d, int w, int rlo, int Gr, int m) {
  const int64_t c = min(max((int64_t)d, (int64_t)rlo - m - w), (int64_t)rlo + Gr + w);
  return (int)(c - w);
}

// BOUNDED: every read has its own column range (nvk_seed_extend_bounded_dev); otherwise the range is the whole strand
// and the compiled kernel is the one nvk_seed_extend_dev always ran.  PATH: a band centre per strip
// (nvk_seed_extend_path_dev) instead of one per read.
template <bool BOUNDED, bool PATH>
__global__ __launch_bounds__(64) void seedext_kernel(SeedArgs a) {
  constexpr int NB = PATH ? 2 : 1;                  // PATH: strip s writes buffer s & 1 and reads the other
  __shared__ int32_t s_ref[64 + 2 * SEED_WMAX];     // r[jbase + x], x = lane + b
  __shared__ int32_t s_h[NB][2 * SEED_WMAX + 2];    // H and F of the previous strip's last row, by band offset
  __shared__ int32_t s_f[NB][2 * SEED_WMAX + 2];
  const int lane = threadIdx.x;
  const int w = a.w, W2 = 2 * w, C = (W2 + 8) / 8;  // dwords per row: ceil((2w + 1) / 8)
  const int O = a.gap_open + a.gap_extend, X = a.gap_extend;
  for (;;) {
    // Control flow stays wave-uniform everywhere: every lane takes part in the atomic (lane 0 adds the 1) and the read,
    // hence every loop bound below, is made scalar with readfirstlane.  (With `if (lane == 0) atomicAdd` the compiler
    // knows the other lanes' value without the atomic and threads their path past it, which runs the lanes'
    // iterations apart around the cross-lane operations below.)
    const int64_t rd = (int64_t)a.r0 + __builtin_amdgcn_readfirstlane(atomicAdd(a.counter, lane == 0 ? 1 : 0));
    if (rd >= a.r1) return;
    __syncthreads();  // (the previous read's last reads of s_h / s_f)
    for (int x = lane; x < 2 * SEED_WMAX + 2; x += 64)
      for (int u = 0; u < NB; u++) {
        s_h[u][x] = 0;
        s_f[u][x] = SEED_NEG;
      }
    const int64_t q0 = a.q_off[rd];
    const int m = (int)(a.q_off[rd + 1] - q0);
    const int st = a.strand[rd];
    const int G = a.G;
    int bh = -1, bi = -1, bj = -1;  // this lane's best cell: largest H, then smallest i, then smallest j
    const int64_t dd = PATH ? 0 : a.diag[rd];
    // the read's columns [rlo, rlo + Gr) on its strand: wave-uniform, as the read is.  Below, j counts columns from
    // rlo, so that the sweep and the traceback compare it with 0 and Gr exactly as they do for the whole reference
    // (rlo = 0, Gr = G); only the staging of the strand and what is reported add rlo back.
    const int rlo = BOUNDED ? __builtin_amdgcn_readfirstlane(a.ref_lo[rd]) : 0;
    const int Gr = BOUNDED ? __builtin_amdgcn_readfirstlane(a.ref_hi[rd]) - rlo : G;
    // any cell at all: the band [d* - w, d* + w] meets the diagonals rlo-(m-1) .. rlo+Gr-1 of the matrix
    // (PATH: every strip is swept, one without a cell like any other)
    const bool meets = (st == 0 || st == 1) && m > 0 && Gr > 0 && dd - w <= rlo + Gr - 1 &&
                       dd + w >= rlo - (int64_t)(m - 1);
    const bool run = PATH ? (st == 0 || st == 1) && m > 0 && Gr > 0 : meets;
    const int lo_read = run ? (int)(dd - w) : 0;  // the band's first diagonal on the strand
    const int lor_read = lo_read - rlo;           // and counted from rlo
    int lo_strip = 0;                             // PATH: the same two of the strip at hand
    const int32_t *sd = PATH ? a.strip_diag + a.strip_off[rd] : nullptr;
    uint32_t *tb = a.tb + a.tb_off[rd];
    const int n_strips = run ? (m + 63) / 64 : 0;
    int d_next = 0;  // PATH: the next strip's centre, asked for one strip ahead of its use
    if constexpr (PATH)
      if (n_strips > 0) d_next = sd[0];
    for (int s = 0; s < n_strips; s++) {
      int delta = 0;  // lo_s - lo_(s-1)
      if constexpr (PATH) {
        const int nlo = path_lo(__builtin_amdgcn_readfirstlane(d_next), w, rlo, Gr, m);
        if (s + 1 < n_strips) d_next = sd[s + 1];
        delta = s > 0 ? nlo - lo_strip : 0;
        lo_strip = nlo;
      }
      const int lo = PATH ? lo_strip : lo_read, lor = PATH ? lo_strip - rlo : lor_read;
      // a band offset of the previous strip's last row as an index of s_h / s_f: outside 0 .. 2w, the empty slot 2w + 1
      // (one unsigned minimum: a negative x is a large unsigned one)
      auto slot = [&](int x) { return (int)min((unsigned)x, (unsigned)(W2 + 1)); };
      const int cur = PATH ? s & 1 : 0, prv = PATH ? cur ^ 1 : 0;
      const int dl = lane == 0 ? delta : 0;  // what moves this lane's up neighbour's offset
      const int i = s * 64 + lane;
      const int jbase = s * 64 + lo;
      __syncthreads();  // (the previous strip's, or read's, last reads of s_ref)
      for (int x = lane; x < 64 + W2; x += 64) s_ref[x] = ref_code(a.reference, G, st, jbase + x);
      __syncthreads();
      const int qi = i < m ? query_code(a.query, q0 + i) : -2;
      const int rows = min(64, m - s * 64);
      const int steps = W2 + 1 + 2 * (rows - 1);
      int h = 0, e = SEED_NEG, f = SEED_NEG;  // this lane's last cell: (i, b-1) at the next step
      int hu_prev = s > 0 ? s_h[prv][PATH ? slot(delta) : 0] : 0;  // lane 0: the diagonal neighbour of its first cell
      uint32_t acc = 0;
      for (int t = 0; t < steps; t++) {
        int hu = dpp_ror1(h), fu = dpp_ror1(f);  // lane l-1's last cell: (i-1, b+1)
        const int b = t - 2 * lane;
        // lane 0's b + 1 (PATH: in the previous strip's offsets): one LDS address for the whole wave
        const int x0 = PATH ? slot(t + 1 + delta) : min(t + 1, W2 + 1);
        const int lh = s_h[prv][x0], lf = s_f[prv][x0];
        hu = lane == 0 ? lh : hu;
        fu = lane == 0 ? lf : fu;
        const int hd = hu_prev;                  // (i-1, b): what arrived one step ago
        hu_prev = hu;
        const int j = i + lor + b;
        const bool cell = b >= 0 && b <= W2 && i < m && j >= 0 && j < Gr;
        const int rj = s_ref[min(max(lane + b, 0), 63 + W2)];
        const int D = ((i > 0 && j > 0) ? hd : 0) + (qi == rj ? a.match : -a.mismatch);
        const bool lok = b >= 1 && j >= 1;       // (i, j-1) is a cell
        const int eo = h - O, ex = e - X;
        const int E = lok ? max(eo, ex) : SEED_NEG;
        // (i-1, j) is a cell (PATH: its offset in the row above, b + 1 + dl, lies in 0 .. 2w; below 0 only where b is)
        const bool uok = i >= 1 && (PATH ? (unsigned)(b + 1 + dl) <= (unsigned)W2 : b + 1 <= W2);
        const int fo = hu - O, fx = fu - X;
        const int F = uok ? max(fo, fx) : SEED_NEG;
        const int best = max(D, max(E, F));
        const int H = best > 0 ? best : 0;
        const uint32_t src = best <= 0 ? 0u : D == best ? 1u : E == best ? 2u : 3u;
        const uint32_t nib = src | (lok && ex > eo ? 4u : 0u) | (uok && fx > fo ? 8u : 0u);
        h = cell ? H : 0;
        e = cell ? E : SEED_NEG;
        f = cell ? F : SEED_NEG;
        if (cell && H > bh) {
          bh = H;
          bi = i;
          bj = j;
        }
        if (b >= 0 && b <= W2) {
          if (lane == 63) {
            s_h[cur][b] = h;
            s_f[cur][b] = f;
          }
          acc |= nib << (4 * (b & 7));
          if ((b & 7) == 7 || b == W2) {
            tb[((int64_t)s * C + (b >> 3)) * 64 + lane] = acc;
            acc = 0;
          }
        }
      }
    }
    // the end cell: lanes own distinct rows, so (H, i) decides
    for (int off = 32; off; off >>= 1) {
      const int oh = __shfl_xor(bh, off), oi = __shfl_xor(bi, off), oj = __shfl_xor(bj, off);
      if (oh > bh || (oh == bh && oi < bi)) {
        bh = oh;
        bi = oi;
        bj = oj;
      }
    }
    bh = __builtin_amdgcn_readfirstlane(bh);
    bi = __builtin_amdgcn_readfirstlane(bi);
    bj = __builtin_amdgcn_readfirstlane(bj);
    const int score = bh > 0 ? bh : 0;
    int cnt = 0;
    __syncthreads();  // every lane's traceback stores before lane 0 reads them
    if (bh >= 0 && score >= a.min_score) {
      // traceback from the end cell, walked by every lane alike (uniform loads); lane 0 stores pair k to slot
      // q0 + m - 1 - k, so they end up ascending
      int i = bi, j = bj, state = 0;  // 0: H, 1: E, 2: F
      int ts = -1, lor_ts = 0;        // PATH: the strip the walk stands in, and its lor
      for (;;) {
        if constexpr (PATH)
          if (i >= 0 && (i >> 6) != ts) {
            ts = i >> 6;
            lor_ts = path_lo(__builtin_amdgcn_readfirstlane(sd[ts]), w, rlo, Gr, m) - rlo;
          }
        const int lor = PATH ? lor_ts : lor_read;
        const int b = j - i - lor;
        // (the rules keep the walk on cells of the band; the guard keeps every access in bounds regardless)
        if (i < 0 || j < 0 || b < 0 || b > W2 || cnt >= m) break;
        const uint32_t nib = (tb[((int64_t)(i >> 6) * C + (b >> 3)) * 64 + (i & 63)] >> (4 * (b & 7))) & 15u;
        if (state == 0) {
          const uint32_t src = nib & 3u;
          if (src == 0) break;
          if (src == 1) {
            if (query_code(a.query, q0 + i) == ref_code(a.reference, G, st, j + rlo)) {
              if (lane == 0) a.out_pairs[q0 + m - 1 - cnt] = make_int2(i, j + rlo);
              cnt++;
            }
            if (i == 0 || j == 0) break;
            i--;
            j--;
          } else {
            state = src == 2 ? 1 : 2;
          }
        } else if (state == 1) {
          j--;
          if (!(nib & 4u)) state = 0;
        } else {
          i--;
          if (!(nib & 8u)) state = 0;
        }
      }
    }
    cnt = __builtin_amdgcn_readfirstlane(__shfl(cnt, 0));
    __syncthreads();  // lane 0's pair stores before the other lanes read them
    // move [q0 + m - cnt, q0 + m) down to [q0, q0 + cnt): every 64 loads of a pass precede its stores, and a pass
    // reads only slots no earlier pass wrote (the source lies at or above the destination)
    const int64_t from = q0 + m - cnt;
    if (from != q0)
      for (int x0 = 0; x0 < cnt; x0 += 64) {
        const int x = x0 + lane;
        int2 p = make_int2(0, 0);
        if (x < cnt) p = a.out_pairs[from + x];
        __syncthreads();
        if (x < cnt) a.out_pairs[q0 + x] = p;
        __syncthreads();
      }
    if (lane == 0)
      *(int4 *)(a.out_hit + 4 * rd) = make_int4(score, bh >= 0 ? bi : -1, bh >= 0 ? bj + rlo : -1, cnt);
  }
}

}  // namespace

// the three entries: ``bounded`` takes ref_lo / ref_hi (checked on the host, as q_off is), the others pass none;
// ``path`` takes strip_off / strip_diag (strip_off checked on the host) and no diag
static int seed_extend(const char *what, bool bounded, bool path, nvk_ctx *ctx, int64_t n_reads, int64_t total_query,
                       const int32_t *query, const int64_t *q_off, const int32_t *reference, int64_t ref_len,
                       const int32_t *strand, const int32_t *diag, int64_t total_strips, const int64_t *strip_off,
                       const int32_t *strip_diag, const int32_t *ref_lo, const int32_t *ref_hi, int band, int match,
                       int mismatch, int gap_open, int gap_extend, int min_score, int32_t *out_hit,
                       int32_t *out_pairs) {
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff || total_query < 0 || ref_len < 0 || ref_len > SEED_MAX_REF) {
    nvk_set_error("%s: n_reads %lld, total_query %lld or ref_len %lld out of range", what, (long long)n_reads,
                  (long long)total_query, (long long)ref_len);
    return NVK_ERR_INVALID;
  }
  if (band > SEED_WMAX) {
    nvk_set_error("%s: band %d is above the compiled limit %d", what, band, SEED_WMAX);
    return NVK_ERR_UNSUPPORTED;
  }
  if (band < 1 || match < 1 || match > 16 || mismatch < 1 || mismatch > 16 || gap_open < 1 || gap_open > 16 ||
      gap_extend < 1 || gap_extend > 16 || min_score < 1) {
    nvk_set_error("%s: band %d, match %d, mismatch %d, gap_open %d, gap_extend %d or min_score %d out of range",
                  what, band, match, mismatch, gap_open, gap_extend, min_score);
    return NVK_ERR_INVALID;
  }
  if (!q_off || (total_query > 0 && !query) || (ref_len > 0 && !reference)) {
    nvk_set_error("%s: NULL query, offsets or reference", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  int rc = nvk_fetch_offsets(ctx, "query", q_off, n_reads, off, "total_query", total_query);
  if (rc) return rc;
  for (int64_t r = 0; r < n_reads; r++)
    if (off[r + 1] - off[r] > SEED_MAX_READ) {
      nvk_set_error("%s: read %lld has %lld bases, above %d", what, (long long)r, (long long)(off[r + 1] - off[r]),
                    SEED_MAX_READ);
      return NVK_ERR_INVALID;
    }
  if (path) {
    if (total_strips < 0 || !strip_off || (total_strips > 0 && !strip_diag)) {
      nvk_set_error("%s: total_strips %lld out of range, or NULL strip offsets or centres", what,
                    (long long)total_strips);
      return NVK_ERR_INVALID;
    }
    std::vector<int64_t> toff;
    if ((rc = nvk_fetch_offsets(ctx, "strip", strip_off, n_reads, toff, "total_strips", total_strips))) return rc;
    for (int64_t r = 0; r < n_reads; r++)
      if (toff[r + 1] - toff[r] != (off[r + 1] - off[r] + 63) / 64) {
        nvk_set_error("%s: read %lld of %lld bases has %lld strips, not %lld", what, (long long)r,
                      (long long)(off[r + 1] - off[r]), (long long)(toff[r + 1] - toff[r]),
                      (long long)((off[r + 1] - off[r] + 63) / 64));
        return NVK_ERR_INVALID;
      }
  }
  if (n_reads == 0) return NVK_OK;
  if (!strand || (!path && !diag) || !out_hit || (total_query > 0 && !out_pairs)) {
    nvk_set_error("%s: NULL strand, diagonal or output", what);
    return NVK_ERR_INVALID;
  }
  if (bounded && (!ref_lo || !ref_hi)) {
    nvk_set_error("%s: NULL ref_lo or ref_hi", what);
    return NVK_ERR_INVALID;
  }
  // the traceback store: per read ceil(m / 64) strips of ceil((2w + 1) / 8) dwords per lane, for the reads that run
  std::vector<int32_t> st((size_t)n_reads);
  NVK_HIP(hipMemcpyAsync(st.data(), strand, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  if (bounded) {
    std::vector<int32_t> lo((size_t)n_reads), hi((size_t)n_reads);
    NVK_HIP(hipMemcpyAsync(lo.data(), ref_lo, lo.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    NVK_HIP(hipMemcpyAsync(hi.data(), ref_hi, hi.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    NVK_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t r = 0; r < n_reads; r++)
      if (st[r] != -1 && (lo[r] < 0 || hi[r] > ref_len || lo[r] > hi[r])) {
        nvk_set_error("%s: read %lld has the reference range [%d, %d), outside 0 <= lo <= hi <= %lld", what,
                      (long long)r, lo[r], hi[r], (long long)ref_len);
        return NVK_ERR_INVALID;
      }
  }
  const int64_t row_dw = (2 * band + 8) / 8 * 64;
  std::vector<int64_t> tb_off((size_t)n_reads + 1, 0);
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t m = off[r + 1] - off[r];
    tb_off[r + 1] = tb_off[r] + (st[r] == 0 || st[r] == 1 ? (m + 63) / 64 * row_dw : 0);
  }
  // chunks of reads whose store fits the cap (a read larger than the cap on its own makes a chunk of one)
  std::vector<int64_t> cut;
  const int64_t need_dw = cut_parts(tb_off, nvk_spill_cap(ctx, WS_SEED_TB) / 4, cut);
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_TB, (size_t)need_dw * 4))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_OFF, ((size_t)n_reads + 1) * sizeof(int64_t) + 64))) return rc;
  int64_t *d_tb_off = (int64_t *)ctx->ws[WS_SEED_OFF];
  int *d_counter = (int *)((char *)ctx->ws[WS_SEED_OFF] + ((size_t)n_reads + 1) * sizeof(int64_t));
  NVK_HIP(hipMemcpyAsync(d_tb_off, tb_off.data(), tb_off.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                         ctx->stream));
  SeedArgs a;
  a.query = query;
  a.q_off = q_off;
  a.reference = reference;
  a.G = (int)ref_len;
  a.strand = strand;
  a.diag = diag;
  a.ref_lo = bounded ? ref_lo : nullptr;
  a.ref_hi = bounded ? ref_hi : nullptr;
  a.strip_diag = path ? strip_diag : nullptr;
  a.strip_off = path ? strip_off : nullptr;
  a.w = band;
  a.match = match;
  a.mismatch = mismatch;
  a.gap_open = gap_open;
  a.gap_extend = gap_extend;
  a.min_score = min_score;
  a.out_hit = out_hit;
  a.out_pairs = (int2 *)out_pairs;
  a.tb_off = d_tb_off;
  a.counter = d_counter;
  {
    TimerScope ts(ctx, NVK_K_SEED);
    for (size_t c = 0; c + 1 < cut.size(); c++) {
      a.r0 = (int)cut[c];
      a.r1 = (int)cut[c + 1];
      a.tb = (uint32_t *)ctx->ws[WS_SEED_TB] - tb_off[cut[c]];
      const int64_t want = a.r1 - a.r0, resident = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 16;
      NVK_HIP(hipMemsetAsync(d_counter, 0, sizeof(int), ctx->stream));
      const dim3 grid((unsigned)(want < resident ? want : resident));
      if (path && bounded)
        hipLaunchKernelGGL((seedext_kernel<true, true>), grid, dim3(64), 0, ctx->stream, a);
      else if (path)
        hipLaunchKernelGGL((seedext_kernel<false, true>), grid, dim3(64), 0, ctx->stream, a);
      else if (bounded)
        hipLaunchKernelGGL((seedext_kernel<true, false>), grid, dim3(64), 0, ctx->stream, a);
      else
        hipLaunchKernelGGL((seedext_kernel<false, false>), grid, dim3(64), 0, ctx->stream, a);
      NVK_HIP(hipGetLastError());
    }
  }
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_seed_extend_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int32_t *query,
                                   const int64_t *q_off, const int32_t *reference, int64_t ref_len,
                                   const int32_t *strand, const int32_t *diag, int band, int match, int mismatch,
                                   int gap_open, int gap_extend, int min_score, int32_t *out_hit,
                                   int32_t *out_pairs) {
  return seed_extend("nvk_seed_extend_dev", false, false, ctx, n_reads, total_query, query, q_off, reference, ref_len,
                     strand, diag, 0, nullptr, nullptr, nullptr, nullptr, band, match, mismatch, gap_open, gap_extend,
                     min_score, out_hit, out_pairs);
}

extern "C" int nvk_seed_extend_bounded_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int32_t *query,
                                           const int64_t *q_off, const int32_t *reference, int64_t ref_len,
                                           const int32_t *strand, const int32_t *diag, const int32_t *ref_lo,
                                           const int32_t *ref_hi, int band, int match, int mismatch, int gap_open,
                                           int gap_extend, int min_score, int32_t *out_hit, int32_t *out_pairs) {
  return seed_extend("nvk_seed_extend_bounded_dev", true, false, ctx, n_reads, total_query, query, q_off, reference,
                     ref_len, strand, diag, 0, nullptr, nullptr, ref_lo, ref_hi, band, match, mismatch, gap_open,
                     gap_extend, min_score, out_hit, out_pairs);
}

extern "C" int nvk_seed_extend_path_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_query, const int32_t *query,
                                        const int64_t *q_off, const int32_t *reference, int64_t ref_len,
                                        const int32_t *strand, int64_t total_strips, const int64_t *strip_off,
                                        const int32_t *strip_diag, const int32_t *ref_lo, const int32_t *ref_hi,
                                        int band, int match, int mismatch, int gap_open, int gap_extend,
                                        int min_score, int32_t *out_hit, int32_t *out_pairs) {
  if ((ref_lo == nullptr) != (ref_hi == nullptr)) {
    nvk_set_error("nvk_seed_extend_path_dev: ref_lo and ref_hi go together, both NULL or neither");
    return NVK_ERR_INVALID;
  }
  return seed_extend("nvk_seed_extend_path_dev", ref_lo != nullptr, true, ctx, n_reads, total_query, query, q_off,
                     reference, ref_len, strand, nullptr, total_strips, strip_off, strip_diag, ref_lo, ref_hi, band,
                     match, mismatch, gap_open, gap_extend, min_score, out_hit, out_pairs);
}
