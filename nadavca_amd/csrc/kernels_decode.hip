// Viterbi decode for decode_batch (nadavca_amd/decode.py): per read the best path of its events over the 4^k k-mer
// states, the bases the path spells and the first event of every base.  The rules are those of include/nadavca_hip.h
// (nvk_viterbi_decode_dev); the CPU restatement the tests hold these kernels to is tests/host_shims/decode_host.cpp,
// which sweeps the full S x E matrix state by state and keeps a flat traceback.
//
// THE SWEEP.  One workgroup per read, T = S / 16 threads (1, 4, 16, 64 or 256 for k = 2..6).  Thread u owns the 16
// consecutive states 16 u .. 16 u + 15: their V, mean, ac and mc stay in registers for the whole read.  The
// predecessors factorise exactly: all 16 states of thread u share the 16 skip predecessors c T + u, and the four states
// 4 g .. 4 g + 3 of the thread share the four step predecessors a (S / 4) + 4 u + g.  So an event costs a thread 16 + 16
// LDS reads of the previous row, five small arg-max reductions (one over 16, four over 4), 16 emissions and 16 LDS
// writes; the stay term never leaves registers.  The arg-maxima are taken on the previous row before the cost is added,
// as the contract writes it, so this form and the restatement's flat one agree on ties.
//
// The row lives in LDS twice (even and odd events), which takes one barrier per event where one buffer would take
// two: a thread may write row i while a slower one still reads row i - 1.  The registers (about 130 VGPRs for the
// thread's own state) hold a CU to two workgroups of 256 threads well before the LDS does, so the second buffer is
// free.  A thread's 16 values are padded by two: the 128-bit writes of eight neighbouring lanes would otherwise all
// fall on the same four banks (thread stride 128 B; with the pad 144 B, which spreads them over all 32): measured 36 ms
// against 50 ms for 10 000 reads.  That makes a row 9 S bytes: 36 KB at k = 6, 72 KB for both.
//
// THE TRACEBACK STORE.  The arg-maxima factorise as the predecessors do: per thread and event one 4-bit c*, four 2-bit
// a* and sixteen 2-bit choices (0 step, 1 stay, 2 skip), 44 bits in one 8-byte word; a row of the store is T words
// written by consecutive threads, 2 KB per event at k = 6.  Event 0 has no row.  Nothing here depends on which reads
// share a launch, so the host cuts a batch into parts whose store fits the workspace cap.
//
// THE WALK BACK is a launch of its own, one thread per read: a chain of one dependent 8-byte load per event, which
// would otherwise hold a whole workgroup's registers and LDS for as long as the sweep itself took.  The walk runs
// from the last event to the first, so it writes the sequence and the bases' events from the END of the read's
// capacity downwards and, once it knows n_bases, moves both down to the start.
//
// The kernels add, multiply and compare doubles and nothing else (no division, log, exp or atomics): with
// -ffp-contract=off every score is the rounded operation the contract writes, on the device as on the host.
#include <vector>

#include "kmer_hmm.h"
#include "nvk_internal.h"
#include "part_cut.h"

namespace {

struct DecodeArgs : HmmIn {
  const int64_t *cap_off;
  double l_stay, l_step, l_skip;
  int32_t *out_hit;  // 4 per read: status, events, bases, end state
  double *out_score;
  int32_t *out_seq, *out_base_event;
  unsigned long long *tb;  // the traceback store: the part's first read starts at word 0
  const int64_t *tb_off;   // per read, its first word in the batch-wide numbering
  int64_t tb_base;         // tb_off of the part's first read
  int r0, r1;              // the part's reads
  int k, central;
};

template <int K>
__global__ __launch_bounds__(KmerHmm<K>::T) void decode_sweep_kernel(DecodeArgs a) {
  constexpr int T = KmerHmm<K>::T, Q = KmerHmm<K>::Q;
  __shared__ __attribute__((aligned(16))) double row[2][KmerHmm<K>::ROW];
  const int u = threadIdx.x;
  const int64_t rd = (int64_t)a.r0 + blockIdx.x;
  const int64_t ev0 = a.ev_off[rd];
  const int E = (int)(a.ev_off[rd + 1] - ev0);
  const int status = hmm_status(a, rd, E);
  if (status != 0) {
    if (u == 0) {
      *(int4 *)(a.out_hit + 4 * rd) = make_int4(status, E, 0, -1);
      a.out_score[rd] = nvk_neg_inf();
    }
    return;
  }
  const double *lev = a.level + ev0;
  const double l_stay = a.l_stay, l_step = a.l_step, l_skip = a.l_skip;
  unsigned long long *tb = a.tb + (a.tb_off[rd] - a.tb_base);

  double V[16], mean[16], ac[16], mc[16];
  double e = lev[0];
  // (hmm_load_table's loop written out: through the helper this kernel comes out with other register counts)
#pragma unroll
  for (int j = 0; j < 16; j++) {
    mean[j] = a.mean[16 * u + j];
    ac[j] = a.ac[16 * u + j];
    mc[j] = a.mc[16 * u + j];
    V[j] = gauss_log(e, mean[j], ac[j], mc[j]);
    row[0][hmm_at(16 * u) + j] = V[j];
  }
  __syncthreads();
  for (int i = 1; i < E; i++) {
    const double *P = row[(i - 1) & 1];
    double *N = row[i & 1];
    e = lev[i];
    // skip: the 16 predecessors c T + u, shared by all the thread's states
    double sk = P[hmm_at(u)];
    unsigned long long word = 0;
#pragma unroll
    for (int c = 1; c < 16; c++) {
      const double v = P[hmm_at(c * T + u)];
      if (v > sk) {
        sk = v;
        word = (unsigned long long)c;
      }
    }
    sk = sk + l_skip;
    // step: per group g of four states the 4 predecessors a Q + 4 u + g
    double st[4];
#pragma unroll
    for (int g = 0; g < 4; g++) st[g] = P[hmm_at(4 * u) + g];
#pragma unroll
    for (int x = 1; x < 4; x++) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const double v = P[hmm_at(x * Q + 4 * u) + g];
        if (v > st[g]) {
          st[g] = v;
          word = (word & ~(3ull << (4 + 2 * g))) | ((unsigned long long)x << (4 + 2 * g));
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 4; g++) st[g] = st[g] + l_step;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const double em = gauss_log(e, mean[j], ac[j], mc[j]);
      const double stay = V[j] + l_stay;
      double v = st[j >> 2];
      unsigned long long w = 0;
      if (stay > v) {
        v = stay;
        w = 1;
      }
      if (sk > v) {
        v = sk;
        w = 2;
      }
      V[j] = v + em;
      word |= w << (12 + 2 * j);
      N[hmm_at(16 * u) + j] = V[j];
    }
    tb[(int64_t)(i - 1) * T + u] = word;
    __syncthreads();
  }
  // the end state: the thread's best (the smallest state among equal ones), then thread 0 over the threads in order
  double best = V[0];
  int at = 0;
#pragma unroll
  for (int j = 1; j < 16; j++)
    if (V[j] > best) {
      best = V[j];
      at = j;
    }
  // (the row of event E - 1 is not read again; the other one is free since the loop's last barrier)
  double *red = row[E & 1];
  red[2 * u] = best;
  red[2 * u + 1] = __longlong_as_double((long long)(16 * u + at));
  __syncthreads();
  if (u == 0) {
    for (int t = 1; t < T; t++)
      if (red[2 * t] > best) {
        best = red[2 * t];
        at = (int)__double_as_longlong(red[2 * t + 1]);
      }
    *(int4 *)(a.out_hit + 4 * rd) = make_int4(0, E, 0, at);
    a.out_score[rd] = best;
  }
}

// one thread per read of the part: the walk back, the sequence and the bases' events
__global__ __launch_bounds__(64) void decode_walk_kernel(DecodeArgs a) {
  const int64_t rd = (int64_t)a.r0 + (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (rd >= a.r1) return;
  int32_t *hit = a.out_hit + 4 * rd;
  if (hit[0] != 0) return;
  const int k = a.k, central = a.central;
  const int T = (1 << (2 * k)) / 16, Q = (1 << (2 * k)) / 4;
  const int E = hit[1];
  int s = hit[3];
  const int64_t cap = a.cap_off[rd + 1] - a.cap_off[rd];
  int32_t *seq = a.out_seq + a.cap_off[rd], *be = a.out_base_event + a.cap_off[rd];
  const unsigned long long *tb = a.tb + (a.tb_off[rd] - a.tb_base);
  // both cursors run down from the capacity's end and write the same number of entries: n_bases <= k + 2 (E - 1)
  int64_t ps = cap - 1, pb = cap - 1;
  for (int x = 0; x < k - 1 - central; x++) be[pb--] = -1;
  for (int i = E - 1; i >= 1; i--) {
    const unsigned long long word = tb[(int64_t)(i - 1) * T + (s >> 4)];
    const int j = s & 15;
    const int w = (int)((word >> (12 + 2 * j)) & 3ull);
    if (w == 1) continue;
    seq[ps--] = s & 3;
    be[pb--] = i;
    if (w == 0) {
      s = (int)((word >> (4 + 2 * (j >> 2))) & 3ull) * Q + (s >> 2);
    } else {
      seq[ps--] = (s >> 2) & 3;
      be[pb--] = -1;
      s = (int)(word & 15ull) * T + (s >> 4);
    }
  }
  be[pb--] = 0;
  for (int x = 0; x < central; x++) be[pb--] = -1;
  for (int x = 0; x < k; x++) seq[ps--] = (s >> (2 * x)) & 3;
  const int64_t n = cap - 1 - ps, from = cap - n;
  if (from > 0)
    for (int64_t x = 0; x < n; x++) {
      seq[x] = seq[from + x];
      be[x] = be[from + x];
    }
  hit[2] = (int32_t)n;
}

}  // namespace

extern "C" int nvk_viterbi_decode_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                                      const int64_t *ev_off, int k, int central, const double *mean, const double *ac,
                                      const double *mc, double l_stay, double l_step, double l_skip,
                                      const int32_t *status_in, int64_t total_cap, const int64_t *cap_off,
                                      int32_t *out_hit, double *out_score, int32_t *out_seq, int32_t *out_base_event,
                                      int64_t *out_parts) {
  const char *what = "nvk_viterbi_decode_dev";
  if (out_parts) *out_parts = 0;
  int rc = hmm_check_entry(what, ctx, k, "central", central, n_reads, total_events, level, ev_off, mean, ac, mc);
  if (rc) return rc;
  if (total_cap < 0) {
    nvk_set_error("%s: n_reads %lld, total_events %lld or total_cap %lld out of range", what, (long long)n_reads,
                  (long long)total_events, (long long)total_cap);
    return NVK_ERR_INVALID;
  }
  if (!cap_off) {
    nvk_set_error("%s: NULL levels, offsets or table", what);
    return NVK_ERR_INVALID;
  }
  if ((rc = check_log_costs(what, "l_stay %g, l_step %g or l_skip %g", {l_stay, l_step, l_skip}))) return rc;
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> eoff, coff;
  if ((rc = nvk_fetch_offsets(ctx, "event", ev_off, n_reads, eoff, "total_events", total_events))) return rc;
  if ((rc = nvk_fetch_offsets(ctx, "capacity", cap_off, n_reads, coff, "total_cap", total_cap))) return rc;
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t E = eoff[r + 1] - eoff[r], cap = coff[r + 1] - coff[r];
    if (E > HMM_MAX_EVENTS) {
      nvk_set_error("%s: read %lld has %lld events, above %d", what, (long long)r, (long long)E, HMM_MAX_EVENTS);
      return NVK_ERR_INVALID;
    }
    if (E >= 1 && cap < k + 2 * (E - 1)) {
      nvk_set_error("%s: read %lld has %lld events and room for %lld bases, below k + 2 (E - 1) = %lld", what,
                    (long long)r, (long long)E, (long long)cap, (long long)(k + 2 * (E - 1)));
      return NVK_ERR_INVALID;
    }
  }
  if (n_reads == 0) return NVK_OK;
  if (!out_hit || !out_score || (total_cap > 0 && (!out_seq || !out_base_event))) {
    nvk_set_error("%s: NULL output", what);
    return NVK_ERR_INVALID;
  }
  // the traceback store, in 64-bit words: per read T words per event but the first.  (A read the kernel skips takes
  // its words all the same: its status is on the device.)
  const int64_t T = ((int64_t)1 << (2 * k)) / 16;
  std::vector<int64_t> tb_off((size_t)n_reads + 1, 0);
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t E = eoff[r + 1] - eoff[r];
    tb_off[r + 1] = tb_off[r] + (E > 1 ? (E - 1) * T : 0);
  }
  // parts of reads whose store fits the cap (a read larger than the cap on its own makes a part of one).  A context
  // without a limit stops at 4 GiB: enough reads per part to fill every CU several times over, and no more of the
  // device than that however large the batch
  int64_t cap_b = nvk_spill_cap(ctx, WS_SEED_TB);
  if (ctx->ws_limit <= 0 && cap_b > ((int64_t)4 << 30)) cap_b = (int64_t)4 << 30;
  std::vector<int64_t> cut;
  const int64_t need_w = cut_parts(tb_off, cap_b / 8, cut);
  // (the seed aligner's traceback workspaces serve: the two never run at once on a context)
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_TB, (size_t)need_w * 8))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_OFF, ((size_t)n_reads + 1) * sizeof(int64_t) + 64))) return rc;
  int64_t *d_tb_off = (int64_t *)ctx->ws[WS_SEED_OFF];
  NVK_HIP(hipMemcpyAsync(d_tb_off, tb_off.data(), tb_off.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                         ctx->stream));
  DecodeArgs a;
  (HmmIn &)a = HmmIn{level, ev_off, mean, ac, mc, status_in};
  a.cap_off = cap_off;
  a.l_stay = l_stay;
  a.l_step = l_step;
  a.l_skip = l_skip;
  a.out_hit = out_hit;
  a.out_score = out_score;
  a.out_seq = out_seq;
  a.out_base_event = out_base_event;
  a.tb_off = d_tb_off;
  a.k = k;
  a.central = central;
  for (size_t c = 0; c + 1 < cut.size(); c++) {
    a.r0 = (int)cut[c];
    a.r1 = (int)cut[c + 1];
    a.tb = (unsigned long long *)ctx->ws[WS_SEED_TB];
    a.tb_base = tb_off[cut[c]];
    hmm_dispatch_k(k, [&](auto kc) {
      constexpr int K = decltype(kc)::value;
      hipLaunchKernelGGL(decode_sweep_kernel<K>, dim3((unsigned)(a.r1 - a.r0)), dim3(KmerHmm<K>::T), 0, ctx->stream, a);
    });
    NVK_HIP(hipGetLastError());
    hipLaunchKernelGGL(decode_walk_kernel, dim3((unsigned)((a.r1 - a.r0 + 63) / 64)), dim3(64), 0, ctx->stream, a);
    NVK_HIP(hipGetLastError());
  }
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  if (out_parts) *out_parts = (int64_t)cut.size() - 1;
  return NVK_OK;
}
