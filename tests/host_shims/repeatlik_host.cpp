// CPU restatement of nvk_repeat_likelihoods_dev (include/nadavca_hip.h; kernel: nadavca_amd/csrc/kernels_repeatlik.hip),
// written in the plain order of the rules over the FULL (E, L, N) trellis of every item: event after event, layer after
// layer, state after state, every source looked up in the row before.  The GPU tests hold the kernel to this bit for
// bit; tests/test_repeat_likelihoods_cpu.py holds this to a plain Python log-domain forward.  Same arguments and
// outputs as the C-ABI call (less the context, the totals and out_ms), on host arrays.  Compile with
// -ffp-contract=off, as the library is.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

namespace {

const double LOG2E = 0x1.71547652b82fep+0;
const double EM_FLOOR = -300.0;

// the fma chain of xm::exp2_frac_horner (csrc/xmath.h): 2^f on [-0.5, 0.5]
double exp2_frac(double f) {
  static const double c[] = {0x1.e9ec1fcb69a7fp-32, 0x1.e6228acd1c6e5p-28, 0x1.b524ebd13a55fp-24, 0x1.62bfc2c86d700p-20,
                             0x1.ffcbfc6da6ed1p-17, 0x1.430913112c61bp-13, 0x1.5d87fe78a3f9cp-10, 0x1.3b2ab6fb9f1a5p-7,
                             0x1.c6b08d704a0c6p-5,  0x1.ebfbdff82c5aep-3,  0x1.62e42fefa39efp-1,  1.0};
  double p = c[0];
  for (int t = 1; t < 12; t++) p = std::fma(p, f, c[t]);
  return p;
}

double EXP(double g) {
  const double y = g * LOG2E;
  const double n = rint(y);
  return ldexp(exp2_frac(y - n), (int)n);
}

int exponent_of(double v) {
  int x = 0;
  (void)frexp(v, &x);
  return x;
}

}  // namespace

extern "C" void repeat_likelihoods_host(int64_t n_items, const int64_t *items, const double *level, const double *mu,
                                        const double *ac, const double *mc, const int64_t *st_off,
                                        const int32_t *chain_par, double w_stay, double w_step, double w_skip,
                                        double w_trim, int layers, const int32_t *status_in, double *out_z,
                                        double *out_x, int32_t *out_status) {
  const int64_t L = layers;
  for (int64_t t = 0; t < n_items; t++) {
    const int64_t ch = items[3 * t], E = items[3 * t + 2] - items[3 * t + 1];
    const int64_t N = st_off[ch + 1] - st_off[ch];
    const double *lev = level + items[3 * t + 1];
    const double *m = mu + st_off[ch], *a = ac + st_off[ch], *c = mc + st_off[ch];
    const int64_t lp_from = chain_par[4 * ch], lp_to = chain_par[4 * ch + 1];
    double *z = out_z + t * L;
    int32_t status = status_in ? status_in[t] : 0;
    if (status == 0 && E == 0) status = 1;
    for (int64_t l = 0; l < L; l++) z[l] = 0.0;
    out_x[t] = 0.0;
    out_status[t] = status;
    if (status != 0) continue;
    std::vector<double> A((size_t)(E * L * N), 0.0), b((size_t)N);
    auto at = [&](int64_t i, int64_t l, int64_t j) -> double {
      return l < 0 || j < 0 ? 0.0 : A[(size_t)((i * L + l) * N + j)];
    };
    auto emit = [&](int64_t i) {
      for (int64_t j = 0; j < N; j++) {
        const double d = lev[i] - m[j];
        b[(size_t)j] = EXP(fmax(a[j] - (d * d) * c[j], EM_FLOOR));
      }
    };
    emit(0);
    A[0] = b[0];
    double o = 1.0;
    int64_t X = 0;
    for (int64_t l = 0; l < L; l++) z[l] = at(0, l, N - 1);
    for (int64_t i = 1; i < E; i++) {
      double top = 0.0;
      for (int64_t l = 0; l < L; l++) {
        top = fmax(top, z[l]);
        for (int64_t j = 0; j < N; j++) top = fmax(top, at(i - 1, l, j));
      }
      const int x = top > 0.0 ? exponent_of(top) : 0;
      o = ldexp(o * w_trim, -x);
      emit(i);
      for (int64_t l = 0; l < L; l++) {
        for (int64_t j = 0; j < N; j++) {
          const double loop = j == lp_to && l >= 1 ? w_step * at(i - 1, l - 1, lp_from) : 0.0;
          const double s = (((w_step * at(i - 1, l, j - 1)) + loop) + (w_stay * at(i - 1, l, j))) +
                           (w_skip * at(i - 1, l, j - 2));
          const double q = l == 0 && j == 0 ? o : 0.0;
          A[(size_t)((i * L + l) * N + j)] = (ldexp(s, -x) + q) * b[(size_t)j];
        }
        z[l] = ldexp(z[l] * w_trim, -x) + at(i, l, N - 1);
      }
      X += x;
    }
    bool any = false;
    for (int64_t l = 0; l < L; l++) any = any || z[l] != 0.0;
    out_x[t] = (double)X;
    out_status[t] = any ? 0 : 2;
  }
}
