// CPU restatement of nvk_signal_locate_dev (include/nadavca_hip.h; kernel: nadavca_amd/csrc/kernels_locate.hip),
// written in the plain order of the rules over the FULL matrix of every (query, target): row after row, no tiles, no
// halo.  The GPU tests hold the kernel to this bit for bit; tests/test_signal_locate_cpu.py holds this to a plain
// Python DP.  Same arguments and outputs as the C-ABI call (less the context, the totals and max_events, which only
// bounds Q there), on host arrays.  Compile with -ffp-contract=off, as the library is.
#include <stddef.h>
#include <stdint.h>

#include <limits>
#include <vector>

extern "C" void signal_locate_host(int64_t n_queries, const double *level, const int64_t *q_off, int64_t n_targets,
                                   const double *mu, const double *ac, const double *mc, const int64_t *col_off,
                                   double l_stay, double l_step, double l_skip, double trim_cost, int64_t n_blocks,
                                   double *out_score, int32_t *out_hit) {
  const double NINF = -std::numeric_limits<double>::infinity();
  const int64_t B = 256;
  for (int64_t q = 0; q < n_queries; q++) {
    const int64_t Q = q_off[q + 1] - q_off[q];
    const double *lev = level + q_off[q];
    int64_t blk0 = 0;
    for (int64_t t = 0; t < n_targets; t++) {
      const int64_t L = col_off[t + 1] - col_off[t];
      const double *m = mu + col_off[t], *a = ac + col_off[t], *c = mc + col_off[t];
      std::vector<double> prev((size_t)L, NINF), cur((size_t)L, NINF), best((size_t)L, NINF);
      std::vector<int32_t> pcol((size_t)L, -1), pev((size_t)L, -1), ccol((size_t)L, -1), cev((size_t)L, -1);
      std::vector<int32_t> bi((size_t)L, -1), bcol((size_t)L, -1), bev((size_t)L, -1);
      for (int64_t i = 0; i < Q; i++) {
        const double e = lev[i];
        const double open = (double)i * trim_cost;
        for (int64_t j = 0; j < L; j++) {
          const double d = e - m[j];
          const double em = a[j] - (d * d) * c[j];
          const double step = (i > 0 && j >= 1 ? prev[j - 1] : NINF) + l_step;
          const double stay = (i > 0 ? prev[j] : NINF) + l_stay;
          const double skip = (i > 0 && j >= 2 ? prev[j - 2] : NINF) + l_skip;
          double v = open;
          int32_t sc = (int32_t)j, se = (int32_t)i;
          if (step > v) v = step, sc = pcol[j - 1], se = pev[j - 1];
          if (stay > v) v = stay, sc = pcol[j], se = pev[j];
          if (skip > v) v = skip, sc = pcol[j - 2], se = pev[j - 2];
          cur[j] = v + em;
          ccol[j] = sc;
          cev[j] = se;
          const double end = cur[j] + (double)(Q - 1 - i) * trim_cost;
          if (end > best[j]) best[j] = end, bi[j] = (int32_t)i, bcol[j] = sc, bev[j] = se;
        }
        prev.swap(cur);
        pcol.swap(ccol);
        pev.swap(cev);
      }
      for (int64_t b = 0; b * B < L; b++) {
        double top = NINF;
        int64_t at = -1;
        for (int64_t j = b * B; j < L && j < (b + 1) * B; j++)
          if (best[j] > top) top = best[j], at = j;
        const int64_t o = q * n_blocks + blk0 + b;
        out_score[o] = top;
        int32_t *hit = out_hit + 4 * o;
        hit[0] = (int32_t)at;
        hit[1] = at < 0 ? -1 : bi[at];
        hit[2] = at < 0 ? -1 : bcol[at];
        hit[3] = at < 0 ? -1 : bev[at];
      }
      blk0 += (L + B - 1) / B;
    }
  }
}
