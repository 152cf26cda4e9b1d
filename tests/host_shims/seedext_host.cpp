// CPU restatement of nvk_seed_extend_dev (include/nadavca_hip.h; kernel: nadavca_amd/csrc/kernels_seedext.hip),
// written cell by cell in the plain order of the rules: for each read, the banded local alignment row by row, the end
// cell, the traceback.  The GPU tests hold the kernel to this bit for bit; tests/test_seed_align_cpu.py holds this to
// a brute-force full-matrix alignment.  Same arguments and outputs as the C-ABI call, on host arrays.
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace {

const int NEG = -(1 << 30);

int qcode(int c) { return c >= 0 && c <= 3 ? c : -2; }

int rcode(const int32_t *ref, int64_t G, int st, int64_t j) {
  if (j < 0 || j >= G) return -1;
  const int c = ref[st ? G - 1 - j : j];
  return c >= 0 && c <= 3 ? (st ? 3 - c : c) : -1;
}

}  // namespace

extern "C" void seedext_host(int64_t n_reads, const int32_t *query, const int64_t *q_off, const int32_t *ref,
                             int64_t G, const int32_t *strand, const int32_t *diag, int w, int match, int mismatch,
                             int gap_open, int gap_extend, int min_score, int32_t *out_hit, int32_t *out_pairs) {
  const int O = gap_open + gap_extend, X = gap_extend;
  const int64_t B = 2 * (int64_t)w + 1;  // band offsets b = j - i - (d* - w)
  for (int64_t rd = 0; rd < n_reads; rd++) {
    const int32_t *q = query + q_off[rd];
    const int64_t m = q_off[rd + 1] - q_off[rd];
    const int st = strand[rd];
    int32_t *hit = out_hit + 4 * rd;
    hit[0] = 0;
    hit[1] = hit[2] = -1;
    hit[3] = 0;
    if (st != 0 && st != 1) continue;
    const int64_t lo = (int64_t)diag[rd] - w;
    auto is_cell = [&](int64_t i, int64_t j) {
      return i >= 0 && i < m && j >= 0 && j < G && j - i >= lo && j - i <= lo + 2 * w;
    };
    std::vector<int> H(m * B, 0), E(m * B, NEG), F(m * B, NEG);
    std::vector<uint8_t> src(m * B, 0), eext(m * B, 0), fext(m * B, 0);
    auto at = [&](int64_t i, int64_t j) { return i * B + (j - i - lo); };
    int64_t bh = -1, bi = -1, bj = -1;
    for (int64_t i = 0; i < m; i++)
      for (int64_t j = std::max<int64_t>(0, i + lo); j <= std::min<int64_t>(G - 1, i + lo + 2 * w); j++) {
        const int64_t c = at(i, j);
        const int s = qcode(q[i]) == rcode(ref, G, st, j) ? match : -mismatch;
        const int D = (i > 0 && j > 0 ? H[at(i - 1, j - 1)] : 0) + s;
        int e = NEG, f = NEG;
        if (is_cell(i, j - 1)) {
          const int64_t l = at(i, j - 1);
          e = std::max(H[l] - O, E[l] - X);
          eext[c] = E[l] - X > H[l] - O;
        }
        if (is_cell(i - 1, j)) {
          const int64_t u = at(i - 1, j);
          f = std::max(H[u] - O, F[u] - X);
          fext[c] = F[u] - X > H[u] - O;
        }
        E[c] = e;
        F[c] = f;
        const int best = std::max(D, std::max(e, f));
        if (best <= 0) {
          H[c] = 0;
          src[c] = 0;
        } else {
          H[c] = best;
          src[c] = D == best ? 1 : e == best ? 2 : 3;
        }
        if (H[c] > bh) {  // rows ascending, then columns: the first of equal H is the smallest (i, j)
          bh = H[c];
          bi = i;
          bj = j;
        }
      }
    if (bh < 0) continue;
    hit[0] = (int32_t)bh;
    hit[1] = (int32_t)bi;
    hit[2] = (int32_t)bj;
    if (bh < min_score) continue;
    std::vector<std::pair<int64_t, int64_t>> pairs;
    int64_t i = bi, j = bj;
    int state = 0;  // 0: H, 1: E, 2: F
    for (;;) {
      const int64_t c = at(i, j);
      if (state == 0) {
        if (src[c] == 0) break;
        if (src[c] == 1) {
          if (qcode(q[i]) == rcode(ref, G, st, j)) pairs.push_back({i, j});
          if (i == 0 || j == 0) break;
          i--;
          j--;
        } else {
          state = src[c] == 2 ? 1 : 2;
        }
      } else if (state == 1) {
        j--;
        if (!eext[c]) state = 0;
      } else {
        i--;
        if (!fext[c]) state = 0;
      }
    }
    std::reverse(pairs.begin(), pairs.end());
    for (size_t k = 0; k < pairs.size(); k++) {
      out_pairs[2 * (q_off[rd] + k)] = (int32_t)pairs[k].first;
      out_pairs[2 * (q_off[rd] + k) + 1] = (int32_t)pairs[k].second;
    }
    hit[3] = (int32_t)pairs.size();
  }
}
