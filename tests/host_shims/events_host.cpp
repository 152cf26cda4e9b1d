// CPU restatements of nvk_event_flags_dev and nvk_event_levels_dev (include/nadavca_hip.h; kernels:
// nadavca_amd/csrc/kernels_events.hip), written in the plain order of the rules: per read the statistic of every
// sample into an array, then the three border conditions sample by sample; per event an ascending sum.  The GPU tests
// hold the kernels to these bit for bit; tests/test_signal_map_cpu.py holds these to plain Python.  Same arguments and
// outputs as the C-ABI calls, on host arrays.  Compile with -ffp-contract=off, as the library is.
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace {

// s(i) of a read of n samples x[0 .. n): w <= i <= n - w, else 0
double statistic(const double *x, int64_t n, int64_t i, int w, double var_floor) {
  if (i < w || i > n - w) return 0.0;
  double sl = 0.0, sr = 0.0;
  for (int t = 0; t < w; t++) sl += x[i - w + t];
  for (int t = 0; t < w; t++) sr += x[i + t];
  const double ml = sl / (double)w, mr = sr / (double)w;
  double vl = 0.0, vr = 0.0;
  for (int t = 0; t < w; t++) {
    const double d = x[i - w + t] - ml;
    vl += d * d;
  }
  for (int t = 0; t < w; t++) {
    const double d = x[i + t] - mr;
    vr += d * d;
  }
  vl = vl / (double)w;
  vr = vr / (double)w;
  const double d = mr - ml;
  return ((double)w * (d * d)) / ((vl + vr) + var_floor);
}

}  // namespace

extern "C" void event_flags_host(int64_t n_reads, const double *signal, const int64_t *sig_off, int window,
                                 double threshold, double var_floor, int32_t *out_flags) {
  for (int64_t rd = 0; rd < n_reads; rd++) {
    const double *x = signal + sig_off[rd];
    const int64_t n = sig_off[rd + 1] - sig_off[rd];
    std::vector<double> s((size_t)n + 1);
    for (int64_t i = 0; i <= n; i++) s[i] = statistic(x, n, i, window, var_floor);
    auto at = [&](int64_t i) { return i >= 0 && i <= n ? s[i] : 0.0; };
    for (int64_t i = 0; i < n; i++) {
      bool border = at(i) >= threshold;
      for (int64_t u = i - window + 1; border && u < i; u++) border = at(i) > at(u);
      for (int64_t u = i + 1; border && u <= i + window - 1; u++) border = at(i) >= at(u);
      out_flags[sig_off[rd] + i] = (i == 0 || border) ? 1 : 0;
    }
  }
}

extern "C" void event_levels_host(int64_t n_reads, int64_t total_signal, const double *signal, const int64_t *sig_off,
                                  int64_t n_events, const int64_t *ev_pos, int32_t *out_start, int32_t *out_len,
                                  double *out_level) {
  int64_t rd = 0;
  for (int64_t e = 0; e < n_events; e++) {
    const int64_t a = ev_pos[e];
    while (rd + 1 < n_reads && sig_off[rd + 1] <= a) rd++;
    int64_t b = e + 1 < n_events ? ev_pos[e + 1] : total_signal;
    if (b > sig_off[rd + 1]) b = sig_off[rd + 1];
    double sum = 0.0;
    for (int64_t g = a; g < b; g++) sum += signal[g];
    out_start[e] = (int32_t)(a - sig_off[rd]);
    out_len[e] = (int32_t)(b - a);
    out_level[e] = sum / (double)(b - a);
  }
}
