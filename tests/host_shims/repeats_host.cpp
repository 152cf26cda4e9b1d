// CPU restatement of nvk_repeat_count_dev (include/nadavca_hip.h; kernel: nadavca_amd/csrc/kernels_repeats.hip),
// written in the plain order of the rules over the FULL E x N matrix of every item, every cell keeping what it carries.
// The GPU tests hold the kernel to this bit for bit; tests/test_repeats_cpu.py holds this to a plain Python DP with an
// explicit traceback.  Same arguments and outputs as the C-ABI call (less the context, the totals and out_ms), on host
// arrays.  Compile with -ffp-contract=off, as the library is.
#include <stddef.h>
#include <stdint.h>

#include <limits>
#include <vector>

namespace {
struct Cell {
  double S, v1, v2;
  int32_t loops, first, i1, i2;
};
}  // namespace

extern "C" void repeat_count_host(int64_t n_items, const int64_t *items, const double *level, const double *mu,
                                  const double *ac, const double *mc, const int64_t *st_off, const int32_t *chain_par,
                                  double l_stay, double l_step, double l_skip, double trim_cost,
                                  const int32_t *status_in, int32_t *out_hit, double *out_score) {
  const double NINF = -std::numeric_limits<double>::infinity();
  const Cell unset = {NINF, NINF, NINF, 0, -1, -1, -1};
  for (int64_t t = 0; t < n_items; t++) {
    const int64_t ch = items[3 * t], E = items[3 * t + 2] - items[3 * t + 1];
    const int64_t N = st_off[ch + 1] - st_off[ch];
    const double *lev = level + items[3 * t + 1];
    const double *m = mu + st_off[ch], *a = ac + st_off[ch], *c = mc + st_off[ch];
    const int64_t lp_from = chain_par[4 * ch], lp_to = chain_par[4 * ch + 1];
    const int64_t m1 = chain_par[4 * ch + 2], m2 = chain_par[4 * ch + 3];
    int32_t *hit = out_hit + 8 * t;
    double *score = out_score + 4 * t;
    int32_t status = status_in ? status_in[t] : 0;
    if (status == 0 && E == 0) status = 1;
    hit[0] = status, hit[1] = (int32_t)E, hit[7] = 0;
    for (int x = 2; x < 7; x++) hit[x] = -1;
    for (int x = 0; x < 4; x++) score[x] = NINF;
    if (status != 0) continue;
    std::vector<Cell> M((size_t)(E * N), unset);
    auto at = [&](int64_t i, int64_t j) -> const Cell & {
      return i < 0 || j < 0 ? unset : M[(size_t)(i * N + j)];
    };
    double best = NINF;
    int64_t last = -1;
    for (int64_t i = 0; i < E; i++) {
      for (int64_t j = 0; j < N; j++) {
        const double d = lev[i] - m[j];
        const double em = a[j] - (d * d) * c[j];
        double v = NINF;
        Cell n = unset;
        int64_t src = j;
        if (j == 0) v = (double)i * trim_cost, n.first = (int32_t)i, src = -1;
        const double step = at(i - 1, j - 1).S + l_step;
        if (step > v) v = step, n = at(i - 1, j - 1), src = j - 1;
        if (j == lp_to) {
          const double loop = at(i - 1, lp_from).S + l_step;
          if (loop > v) v = loop, n = at(i - 1, lp_from), n.loops += 1, src = lp_from;
        }
        const double stay = at(i - 1, j).S + l_stay;
        if (stay > v) v = stay, n = at(i - 1, j), src = j;
        const double skip = at(i - 1, j - 2).S + l_skip;
        if (skip > v) v = skip, n = at(i - 1, j - 2), src = j - 2;
        if (j >= m1 && src < m1) n.v1 = v, n.i1 = (int32_t)i;
        if (j >= m2 && src < m2) n.v2 = v, n.i2 = (int32_t)i;
        n.S = v + em;
        M[(size_t)(i * N + j)] = n;
      }
      const double end = at(i, N - 1).S + (double)(E - 1 - i) * trim_cost;
      if (end > best) best = end, last = i;
    }
    if (last < 0) {
      hit[0] = 2;
      continue;
    }
    const Cell &f = at(last, N - 1);
    hit[2] = f.first, hit[3] = (int32_t)last, hit[4] = f.loops, hit[5] = f.i1, hit[6] = f.i2;
    score[0] = best, score[1] = f.S, score[2] = f.v1, score[3] = f.v2;
  }
}
