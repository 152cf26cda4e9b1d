// CPU restatement of nvk_viterbi_decode_dev (include/nadavca_hip.h; kernels: nadavca_amd/csrc/kernels_decode.hip),
// written in the plain order of the rules: the full S x E matrix, state after state, every candidate looked up flat,
// and a flat traceback (per cell its predecessor and how many bases the move adds); the path is then read FORWARDS,
// event 0 first.  The GPU tests hold the kernels to this bit for bit; tests/test_decode_cpu.py holds this to a plain
// Python Viterbi.  Same arguments and outputs as the C-ABI call (less the context, the totals and out_parts), on host
// arrays.  Compile with -ffp-contract=off, as the library is.
#include <stddef.h>
#include <stdint.h>

#include <limits>
#include <vector>

extern "C" void viterbi_decode_host(int64_t n_reads, const double *level, const int64_t *ev_off, int k, int central,
                                    const double *mean, const double *ac, const double *mc, double l_stay,
                                    double l_step, double l_skip, const int32_t *status_in, const int64_t *cap_off,
                                    int32_t *out_hit, double *out_score, int32_t *out_seq, int32_t *out_base_event) {
  const double NINF = -std::numeric_limits<double>::infinity();
  const int64_t S = (int64_t)1 << (2 * k), Q = S / 4, T = S / 16;
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t E = ev_off[r + 1] - ev_off[r];
    const double *lev = level + ev_off[r];
    int32_t *hit = out_hit + 4 * r;
    int32_t status = status_in ? status_in[r] : 0;
    if (status == 0 && E == 0) status = 1;
    if (status != 0) {
      hit[0] = status, hit[1] = (int32_t)E, hit[2] = 0, hit[3] = -1;
      out_score[r] = NINF;
      continue;
    }
    std::vector<double> prev((size_t)S), cur((size_t)S);
    std::vector<int32_t> from((size_t)(E * S), -1);  // the predecessor of cell (i, s)
    std::vector<int8_t> adds((size_t)(E * S), 0);    // bases the move into (i, s) adds: 1 step, 0 stay, 2 skip
    for (int64_t i = 0; i < E; i++) {
      const double e = lev[i];
      for (int64_t s = 0; s < S; s++) {
        const double em = ac[s] - ((e - mean[s]) * (e - mean[s])) * mc[s];
        if (i == 0) {
          cur[s] = em;
          continue;
        }
        int64_t pa = s / 4, pc = s / 16;
        for (int64_t a = 1; a < 4; a++)
          if (prev[a * Q + s / 4] > prev[pa]) pa = a * Q + s / 4;
        for (int64_t c = 1; c < 16; c++)
          if (prev[c * T + s / 16] > prev[pc]) pc = c * T + s / 16;
        const double step = prev[pa] + l_step, stay = prev[s] + l_stay, skip = prev[pc] + l_skip;
        double v = step;
        int64_t p = pa;
        int8_t n = 1;
        if (stay > v) v = stay, p = s, n = 0;
        if (skip > v) v = skip, p = pc, n = 2;
        cur[s] = v + em;
        from[(size_t)(i * S + s)] = (int32_t)p;
        adds[(size_t)(i * S + s)] = n;
      }
      prev.swap(cur);
    }
    int64_t end = 0;
    for (int64_t s = 1; s < S; s++)
      if (prev[s] > prev[end]) end = s;
    out_score[r] = prev[end];
    // the path, backwards, then everything else forwards
    std::vector<int64_t> path((size_t)E);
    path[(size_t)(E - 1)] = end;
    for (int64_t i = E - 1; i >= 1; i--) path[(size_t)(i - 1)] = from[(size_t)(i * S + path[(size_t)i])];
    int32_t *seq = out_seq + cap_off[r], *be = out_base_event + cap_off[r];
    int64_t n = 0;
    for (int t = k - 1; t >= 0; t--) seq[n++] = (int32_t)((path[0] >> (2 * t)) & 3);
    for (int64_t i = 1; i < E; i++) {
      const int64_t s = path[(size_t)i];
      const int8_t m = adds[(size_t)(i * S + s)];
      if (m == 2) seq[n++] = (int32_t)((s / 4) % 4);
      if (m >= 1) seq[n++] = (int32_t)(s % 4);
    }
    for (int64_t b = 0; b < n; b++) be[b] = -1;
    int64_t owner = central;
    be[owner] = 0;
    for (int64_t i = 1; i < E; i++) {
      const int8_t m = adds[(size_t)(i * S + path[(size_t)i])];
      if (m == 0) continue;
      owner += m;
      be[owner] = (int32_t)i;
    }
    hit[0] = 0, hit[1] = (int32_t)E, hit[2] = (int32_t)n, hit[3] = (int32_t)end;
  }
}
