// CPU restatement of nvk_kmer_expectations_dev (include/nadavca_hip.h; kernels: nadavca_amd/csrc/kernels_posterior.hip),
// written in the plain order of the rules as posterior_host.cpp is: the full S x E matrices A and B, state after state,
// every predecessor and successor looked up flat, the sums over all states as the contract orders them (blocks of 16
// ascending, then the butterfly over the blocks on an array), the sums over events descending.  The GPU tests hold the
// kernels to this bit for bit; tests/test_expectation_cpu.py holds this to a plain-numpy log-domain Baum-Welch.  Same
// arguments and outputs as the C-ABI call (less the context, the totals, out_parts and out_ms), on host arrays.
// Compile with -ffp-contract=off, as the library is.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
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

// the sum over all states of v[0..S): blocks of 16 ascending, the butterfly over the T blocks, four groups of 64 joined
// as (g0 + g1) + (g2 + g3)
double sum_states(const std::vector<double> &v) {
  const int64_t S = (int64_t)v.size(), T = S / 16, W = std::min<int64_t>(T, 64);
  std::vector<double> blk((size_t)T);
  for (int64_t u = 0; u < T; u++) {
    double acc = v[(size_t)(16 * u)];
    for (int64_t j = 1; j < 16; j++) acc = acc + v[(size_t)(16 * u + j)];
    blk[(size_t)u] = acc;
  }
  for (int64_t d = W / 2; d >= 1; d /= 2) {
    std::vector<double> next((size_t)T);
    for (int64_t u = 0; u < T; u++) next[(size_t)u] = blk[(size_t)u] + blk[(size_t)(u ^ d)];
    blk.swap(next);
  }
  if (T <= 64) return blk[0];
  return (blk[0] + blk[64]) + (blk[128] + blk[192]);
}

}  // namespace

extern "C" void kmer_expectations_host(int64_t n_reads, const double *level, const int64_t *ev_off, int k,
                                       const double *mean, const double *ac, const double *mc, double w_stay,
                                       double w_step, double w_skip, const int32_t *status_in, double *out_stats,
                                       double *out_z, int32_t *out_status) {
  const int64_t S = (int64_t)1 << (2 * k), Q = S / 4, T = S / 16;
  for (int64_t r = 0; r < n_reads; r++) {
    const int64_t E = ev_off[r + 1] - ev_off[r];
    const double *lev = level + ev_off[r];
    int32_t status = status_in ? status_in[r] : 0;
    if (status == 0 && E == 0) status = 1;
    out_status[r] = status;
    if (status != 0) {
      out_z[2 * r] = out_z[2 * r + 1] = 0.0;
      continue;
    }
    std::vector<double> b((size_t)(E * S)), A((size_t)(E * S)), B((size_t)(E * S));
    std::vector<char> floored((size_t)E);
    for (int64_t i = 0; i < E; i++) {
      double top = -INFINITY;
      for (int64_t s = 0; s < S; s++) {
        const double e = lev[i];
        const double em = ac[s] - ((e - mean[s]) * (e - mean[s])) * mc[s];
        top = std::max(top, em);
        b[(size_t)(i * S + s)] = EXP(std::max(em, EM_FLOOR));
      }
      floored[(size_t)i] = top <= EM_FLOOR;
    }
    // forward
    int64_t X = 0;
    for (int64_t s = 0; s < S; s++) A[(size_t)s] = b[(size_t)s];
    for (int64_t i = 1; i < E; i++) {
      const double *P = &A[(size_t)((i - 1) * S)];
      const int x = exponent_of(*std::max_element(P, P + S));
      for (int64_t s = 0; s < S; s++) {
        const int64_t q = s / 4, h = s / 16;
        const double sum4 = ((P[0 * Q + q] + P[1 * Q + q]) + P[2 * Q + q]) + P[3 * Q + q];
        double sum16 = P[h];
        for (int64_t c = 1; c < 16; c++) sum16 = sum16 + P[c * T + h];
        const double t = ((w_step * sum4) + (w_stay * P[s])) + (w_skip * sum16);
        A[(size_t)(i * S + s)] = ldexp(t, -x) * b[(size_t)(i * S + s)];
      }
      X += x;
    }
    // backward, keeping W, G4 and G16 of every event but the first
    std::vector<double> Wm((size_t)(E * S)), G4m((size_t)(E * Q)), G16m((size_t)(E * T));
    for (int64_t s = 0; s < S; s++) B[(size_t)((E - 1) * S + s)] = 1.0;
    for (int64_t i = E - 2; i >= 0; i--) {
      const double *Bn = &B[(size_t)((i + 1) * S)];
      double *W = &Wm[(size_t)((i + 1) * S)], *G4 = &G4m[(size_t)((i + 1) * Q)], *G16 = &G16m[(size_t)((i + 1) * T)];
      for (int64_t s = 0; s < S; s++) W[s] = Bn[s] * b[(size_t)((i + 1) * S + s)];
      for (int64_t q = 0; q < Q; q++) G4[q] = ((W[4 * q] + W[4 * q + 1]) + W[4 * q + 2]) + W[4 * q + 3];
      for (int64_t h = 0; h < T; h++) G16[h] = ((G4[4 * h] + G4[4 * h + 1]) + G4[4 * h + 2]) + G4[4 * h + 3];
      const int y = exponent_of(*std::max_element(Bn, Bn + S));
      for (int64_t s = 0; s < S; s++)
        B[(size_t)(i * S + s)] = ldexp(((w_step * G4[s % Q]) + (w_stay * W[s])) + (w_skip * G16[s % T]), -y);
    }
    // the expected counts and moments, the events descending
    double M0 = 0.0, Mx = 0.0, Mxx = 0.0, Mm = 0.0, Mxm = 0.0, Mmm = 0.0, Nstay = 0.0, Nstep = 0.0, Nskip = 0.0;
    double n_floored = 0.0;
    std::vector<double> ab((size_t)S), t0((size_t)S), t1((size_t)S), t2((size_t)S);
    for (int64_t i = E - 1; i >= 0; i--) {
      const double *Ai = &A[(size_t)(i * S)];
      for (int64_t s = 0; s < S; s++) {
        ab[(size_t)s] = Ai[s] * B[(size_t)(i * S + s)];
        t0[(size_t)s] = ab[(size_t)s] * mc[s];
        t1[(size_t)s] = t0[(size_t)s] * mean[s];
        t2[(size_t)s] = t1[(size_t)s] * mean[s];
      }
      const double D = sum_states(ab), m0 = sum_states(t0), m1 = sum_states(t1), m2 = sum_states(t2);
      const double x = lev[i];
      const double g0 = m0 / D, g1 = m1 / D, g2 = m2 / D;
      M0 = M0 + g0;
      Mx = Mx + g0 * x;
      Mxx = Mxx + (g0 * x) * x;
      Mm = Mm + g1;
      Mxm = Mxm + g1 * x;
      Mmm = Mmm + g2;
      if (floored[(size_t)i]) n_floored = n_floored + 1.0;
      if (i < E - 1) {
        const double *W = &Wm[(size_t)((i + 1) * S)], *G4 = &G4m[(size_t)((i + 1) * Q)];
        const double *G16 = &G16m[(size_t)((i + 1) * T)];
        for (int64_t s = 0; s < S; s++) {
          t0[(size_t)s] = Ai[s] * (w_stay * W[s]);
          t1[(size_t)s] = Ai[s] * (w_step * G4[s % Q]);
          t2[(size_t)s] = Ai[s] * (w_skip * G16[s % T]);
        }
        const double n_stay = sum_states(t0), n_step = sum_states(t1), n_skip = sum_states(t2);
        const double total = (n_stay + n_step) + n_skip;
        Nstay = Nstay + n_stay / total;
        Nstep = Nstep + n_step / total;
        Nskip = Nskip + n_skip / total;
      }
    }
    double *out = out_stats + 10 * r;
    out[0] = M0, out[1] = Mx, out[2] = Mxx, out[3] = Mm, out[4] = Mxm, out[5] = Mmm;
    out[6] = Nstay, out[7] = Nstep, out[8] = Nskip, out[9] = n_floored;
    out_z[2 * r] = sum_states(std::vector<double>(&A[(size_t)((E - 1) * S)], &A[(size_t)((E - 1) * S)] + S));
    out_z[2 * r + 1] = (double)X;
  }
}
