// CPU restatements of nvk_seed_chain_dev and nvk_seed_extend_path_dev (include/nadavca_hip.h; kernels:
// nadavca_amd/csrc/kernels_seedchain.hip and the path form of kernels_seedext.hip), written in the plain order of the
// rules: the chain's DP seed by seed over the lookback window, its end, the backtrack, then per strip a search of the
// anchors for the nearest one; the banded alignment row by row with each row's own band, the end cell, the traceback.
// The GPU tests hold the kernels to these bit for bit; tests/test_seed_chain_cpu.py holds these to plain Python and to
// seedext_host.cpp.  Same arguments and outputs as the C-ABI calls, on host arrays.
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

extern "C" void seedchain_host(int64_t n_reads, const int64_t *q_off, const int32_t *strand, const int64_t *seed_off,
                               const int32_t *seed_i, const int32_t *seed_p, int k, int w, int max_gap, int lookback,
                               const int64_t *strip_off, int32_t *strip_diag, int32_t *out_chain) {
  for (int64_t rd = 0; rd < n_reads; rd++) {
    out_chain[2 * rd] = out_chain[2 * rd + 1] = 0;
    const int64_t n = seed_off[rd + 1] - seed_off[rd], m = q_off[rd + 1] - q_off[rd];
    if ((strand[rd] != 0 && strand[rd] != 1) || n == 0) continue;
    const int32_t *si = seed_i + seed_off[rd], *sp = seed_p + seed_off[rd];
    std::vector<int64_t> f(n), pred(n);
    int64_t end = 0;
    for (int64_t t = 0; t < n; t++) {
      f[t] = k;
      pred[t] = -1;
      for (int64_t u = std::max<int64_t>(0, t - lookback); u < t; u++) {
        const int64_t di = (int64_t)si[t] - si[u], dp = (int64_t)sp[t] - sp[u];
        const int64_t gap = dp > di ? dp - di : di - dp;
        if (di <= 0 || di > max_gap || dp <= 0 || dp > max_gap || gap > w) continue;
        const int64_t cand = f[u] + std::min<int64_t>(std::min(di, dp), k) - gap;
        if (cand > k && cand >= f[t]) {  // u ascending: on a tie the later, nearer one stays
          f[t] = cand;
          pred[t] = u;
        }
      }
      if (f[t] > f[end]) end = t;
    }
    std::vector<int64_t> anchors;
    for (int64_t t = end; t >= 0; t = pred[t]) anchors.push_back(t);
    std::reverse(anchors.begin(), anchors.end());
    out_chain[2 * rd] = (int32_t)f[end];
    out_chain[2 * rd + 1] = (int32_t)anchors.size();
    for (int64_t s = 0; s < (m + 63) / 64; s++) {
      const int64_t c = 64 * s + 32;
      int64_t best = anchors[0];
      for (int64_t a : anchors) {  // i ascending along the chain: a strict < keeps the smaller i on a tie
        const int64_t da = si[a] > c ? si[a] - c : c - si[a], db = si[best] > c ? si[best] - c : c - si[best];
        if (da < db) best = a;
      }
      strip_diag[strip_off[rd] + s] = sp[best] - si[best];
    }
  }
}

// ref_lo / ref_hi: both null (the whole strand) or one range per read
extern "C" void seedext_path_host(int64_t n_reads, const int32_t *query, const int64_t *q_off, const int32_t *ref,
                                  int64_t G, const int32_t *strand, const int64_t *strip_off,
                                  const int32_t *strip_diag, const int32_t *ref_lo, const int32_t *ref_hi, int w,
                                  int match, int mismatch, int gap_open, int gap_extend, int min_score,
                                  int32_t *out_hit, int32_t *out_pairs) {
  const int O = gap_open + gap_extend, X = gap_extend;
  const int64_t B = 2 * (int64_t)w + 1;  // band offsets b = j - i - (d(i) - w)
  for (int64_t rd = 0; rd < n_reads; rd++) {
    const int32_t *q = query + q_off[rd];
    const int64_t m = q_off[rd + 1] - q_off[rd];
    const int st = strand[rd];
    int32_t *hit = out_hit + 4 * rd;
    hit[0] = 0;
    hit[1] = hit[2] = -1;
    hit[3] = 0;
    if (st != 0 && st != 1) continue;
    const int64_t jlo = ref_lo ? ref_lo[rd] : 0, jhi = ref_hi ? ref_hi[rd] : G;
    const int32_t *centre = strip_diag + strip_off[rd];
    auto lo = [&](int64_t i) { return (int64_t)centre[i / 64] - w; };
    auto is_cell = [&](int64_t i, int64_t j) {
      return i >= 0 && i < m && j >= jlo && j < jhi && j - i >= lo(i) && j - i <= lo(i) + 2 * w;
    };
    std::vector<int> H(m * B, 0), E(m * B, NEG), F(m * B, NEG);
    std::vector<uint8_t> src(m * B, 0), eext(m * B, 0), fext(m * B, 0);
    auto at = [&](int64_t i, int64_t j) { return i * B + (j - i - lo(i)); };
    int64_t bh = -1, bi = -1, bj = -1;
    for (int64_t i = 0; i < m; i++)
      for (int64_t j = std::max<int64_t>(jlo, i + lo(i)); j <= std::min<int64_t>(jhi - 1, i + lo(i) + 2 * w); j++) {
        const int64_t c = at(i, j);
        const int s = qcode(q[i]) == rcode(ref, G, st, j) ? match : -mismatch;
        const int D = (is_cell(i - 1, j - 1) ? H[at(i - 1, j - 1)] : 0) + s;
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
      if (!is_cell(i, j)) break;  // (the rules keep the walk on cells: E and F are taken only from cells)
      const int64_t c = at(i, j);
      if (state == 0) {
        if (src[c] == 0) break;
        if (src[c] == 1) {
          if (qcode(q[i]) == rcode(ref, G, st, j)) pairs.push_back({i, j});
          if (i == 0 || j == jlo) break;
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
    for (size_t x = 0; x < pairs.size(); x++) {
      out_pairs[2 * (q_off[rd] + x)] = (int32_t)pairs[x].first;
      out_pairs[2 * (q_off[rd] + x) + 1] = (int32_t)pairs[x].second;
    }
    hit[3] = (int32_t)pairs.size();
  }
}
