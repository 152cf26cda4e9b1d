// CPU restatement of nvk_event_align_dev (include/nadavca_hip.h; kernel: nadavca_amd/csrc/kernels_eventalign.hip),
// written in the plain order of the rules: band after band with every band's cells, corner and moves kept in arrays,
// the end cell, the walk back.  The GPU tests hold the kernel to this bit for bit; tests/test_signal_map_cpu.py holds
// this to a full-matrix Python DP.  Same arguments and outputs as the C-ABI call, on host arrays.  Compile with
// -ffp-contract=off, as the library is.  One argument more than the C-ABI call: out_corner (may be null; for a batch of
// ONE read) receives the corner (event, base) of each of the read's E + K + 1 bands, which the library keeps to itself.
#include <stddef.h>
#include <stdint.h>

#include <limits>
#include <vector>

extern "C" void event_align_host(int64_t n_reads, const double *level, const int64_t *ev_off, const double *mu,
                                 const double *ac, const double *mc, const int64_t *base_off, const double *l_stay,
                                 const double *l_step, const int32_t *status_in, int band, double trim_cost,
                                 double skip_cost, int32_t *out_hit, double *out_score, int32_t *out_base_event,
                                 int32_t *out_corner) {
  const double NINF = -std::numeric_limits<double>::infinity();
  const int H = band / 2;
  for (int64_t rd = 0; rd < n_reads; rd++) {
    const int64_t E = ev_off[rd + 1] - ev_off[rd], K = base_off[rd + 1] - base_off[rd];
    const double *lev = level + ev_off[rd];
    const double *m = mu + base_off[rd], *a = ac + base_off[rd], *c = mc + base_off[rd];
    int32_t *hit = out_hit + 4 * rd, *be = out_base_event + base_off[rd];
    for (int64_t j = 0; j < K; j++) be[j] = -1;
    hit[0] = status_in && status_in[rd] != 0 ? status_in[rd] : (E == 0 || K == 0) ? 1 : 0;
    hit[1] = (int32_t)E;
    hit[2] = hit[3] = -1;
    out_score[rd] = NINF;
    if (hit[0] != 0) continue;
    const int64_t nb = E + K + 1;
    std::vector<int64_t> lle((size_t)nb), llk((size_t)nb);          // the band's corner: its cell at offset 0
    std::vector<double> val((size_t)nb * band);
    std::vector<uint8_t> mv((size_t)nb * band, 0);
    auto cell = [&](int64_t b, int64_t i, int64_t j) {              // a cell's score as a neighbour sees it
      if (b < 0) return NINF;
      const int64_t o = j - llk[b];
      if (o < 0 || o >= band || lle[b] - o != i) return NINF;
      return val[(size_t)b * band + o];
    };
    double best = NINF;
    int64_t best_i = -1;
    for (int64_t b = 0; b < nb; b++) {
      if (b == 0) {
        lle[b] = H - 1;
        llk[b] = -1 - H;
      } else {
        bool right = false;
        if (b >= 2) {
          const double ll = val[(size_t)(b - 1) * band], ur = val[(size_t)(b - 1) * band + band - 1];
          right = (ll == NINF && ur == NINF) ? (b & 1) != 0 : ll < ur;
        }
        lle[b] = lle[b - 1] + (right ? 0 : 1);
        llk[b] = llk[b - 1] + (right ? 1 : 0);
      }
      for (int o = 0; o < band; o++) {
        const int64_t i = lle[b] - o, j = llk[b] + o;
        double v = NINF;
        if (j == -1 && i >= -1 && i < E) {
          v = (double)(i + 1) * trim_cost;  // the trimmed column: steers the band, feeds no cell
        } else if (i >= 0 && i < E && j >= 0 && j < K) {
          const double d = lev[i] - m[j];
          const double em = a[j] - d * d * c[j];
          const double src = j == 0 ? (double)i * trim_cost : cell(b - 2, i - 1, j - 1);
          const double step = (src + l_step[rd]) + em;
          const double stay = (cell(b - 1, i - 1, j) + l_stay[rd]) + em;
          const double skip = j > 0 ? cell(b - 1, i, j - 1) + skip_cost : NINF;
          v = step;
          uint8_t w = 0;
          if (stay > v) {
            v = stay;
            w = 1;
          }
          if (skip > v) {
            v = skip;
            w = 2;
          }
          mv[(size_t)b * band + o] = w;
          if (j == K - 1) {
            const double end = v + (double)(E - 1 - i) * trim_cost;
            if (end > best || (end == best && best_i >= 0 && i < best_i)) {
              best = end;
              best_i = i;
            }
          }
        }
        val[(size_t)b * band + o] = v;
      }
    }
    if (out_corner)
      for (int64_t b = 0; b < nb; b++) {
        out_corner[2 * b] = (int32_t)lle[b];
        out_corner[2 * b + 1] = (int32_t)llk[b];
      }
    if (best_i < 0) {
      hit[0] = 2;
      continue;
    }
    // the walk back from (best_i, K - 1); a base's first event is the smallest i of its cells entered by step or stay
    int64_t i = best_i, j = K - 1, first = -1, skipped = 0;
    int32_t fe = -1;
    for (int64_t guard = 0; guard < nb; guard++) {
      const int64_t b = i + j + 2, o = j - llk[b];
      if (i < 0 || o < 0 || o >= band || lle[b] - o != i) break;  // (the moves keep the walk on cells of the bands)
      const uint8_t w = mv[(size_t)b * band + o];
      if (w == 2) {
        skipped++;
        be[j] = fe;
        fe = -1;
        j--;
        continue;
      }
      fe = (int32_t)i;
      if (w == 1) {
        if (i == 0) break;
        i--;
        continue;
      }
      be[j] = fe;
      fe = -1;
      if (j == 0) {
        first = i;
        break;
      }
      i--;
      j--;
    }
    if (first < 0 || 8 * skipped > K) {  // lost: the walk left the bands, or more than an eighth of the bases has no event
      for (int64_t x = 0; x < K; x++) be[x] = -1;
      hit[0] = 2;
      continue;
    }
    hit[2] = (int32_t)first;
    hit[3] = (int32_t)best_i;
    out_score[rd] = best;
  }
}
