// CPU restatement of nvk_kmer_state_moments_dev (include/nadavca_hip.h; kernels: nadavca_amd/csrc/kernels_posterior.hip),
// written in the plain order of the rules as expect_host.cpp is: the full S x E matrices A and B, state after state,
// every predecessor and successor looked up flat, D as the contract orders a sum over all states (blocks of 16
// ascending, then the butterfly over the blocks on an array), the events descending, the reads ascending.  The GPU
// tests hold the kernels to this bit for bit; tests/test_state_moments_cpu.py holds this to a plain-numpy log-domain
// forward-backward.  kmer_state_moments_host writes every read's own G (so that the reads can be spread over threads)
// and state_moments_total_host chains them into the batch's totals.  Compile with -ffp-contract=off, as the library is.
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
double sum_states(const double *v, int64_t S) {
  const int64_t T = S / 16, W = std::min<int64_t>(T, 64);
  std::vector<double> blk((size_t)T);
  for (int64_t u = 0; u < T; u++) {
    double acc = v[16 * u];
    for (int64_t j = 1; j < 16; j++) acc = acc + v[16 * u + j];
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

// out_read f64[n_reads][3][4^k]: per read G0, G1 and G2; a read that is not processed keeps what the caller put there
extern "C" void kmer_state_moments_host(int64_t n_reads, const double *level, const int64_t *ev_off, int k,
                                        const double *mean, const double *ac, const double *mc, double w_stay,
                                        double w_step, double w_skip, const int32_t *status_in, double *out_read,
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
    for (int64_t i = 0; i < E; i++)
      for (int64_t s = 0; s < S; s++) {
        const double e = lev[i];
        const double em = ac[s] - ((e - mean[s]) * (e - mean[s])) * mc[s];
        b[(size_t)(i * S + s)] = EXP(std::max(em, EM_FLOOR));
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
    // backward
    std::vector<double> W((size_t)S), G4((size_t)Q), G16((size_t)T);
    for (int64_t s = 0; s < S; s++) B[(size_t)((E - 1) * S + s)] = 1.0;
    for (int64_t i = E - 2; i >= 0; i--) {
      const double *Bn = &B[(size_t)((i + 1) * S)];
      for (int64_t s = 0; s < S; s++) W[(size_t)s] = Bn[s] * b[(size_t)((i + 1) * S + s)];
      for (int64_t q = 0; q < Q; q++) G4[(size_t)q] = ((W[4 * q] + W[4 * q + 1]) + W[4 * q + 2]) + W[4 * q + 3];
      for (int64_t h = 0; h < T; h++) G16[(size_t)h] = ((G4[4 * h] + G4[4 * h + 1]) + G4[4 * h + 2]) + G4[4 * h + 3];
      const int y = exponent_of(*std::max_element(Bn, Bn + S));
      for (int64_t s = 0; s < S; s++)
        B[(size_t)(i * S + s)] =
            ldexp(((w_step * G4[(size_t)(s % Q)]) + (w_stay * W[(size_t)s])) + (w_skip * G16[(size_t)(s % T)]), -y);
    }
    // the per-state moments, the events descending
    double *G0 = out_read + r * 3 * S, *G1 = G0 + S, *G2 = G1 + S;
    for (int64_t s = 0; s < 3 * S; s++) G0[s] = 0.0;
    std::vector<double> ab((size_t)S);
    for (int64_t i = E - 1; i >= 0; i--) {
      for (int64_t s = 0; s < S; s++) ab[(size_t)s] = A[(size_t)(i * S + s)] * B[(size_t)(i * S + s)];
      const double D = sum_states(ab.data(), S);
      const double inv = 1.0 / D;
      const double x = lev[i];
      for (int64_t s = 0; s < S; s++) {
        const double g = ab[(size_t)s] * inv;
        G0[s] = G0[s] + g;
        G1[s] = G1[s] + g * x;
        G2[s] = G2[s] + (g * x) * x;
      }
    }
    out_z[2 * r] = sum_states(&A[(size_t)((E - 1) * S)], S);
    out_z[2 * r + 1] = (double)X;
  }
}

// the batch's totals: tot starts at 0.0 and takes the reads with status 0 in ascending order; n3 = 3 * 4^k
extern "C" void state_moments_total_host(int64_t n_reads, int64_t n3, const double *per_read, const int32_t *status,
                                         double *out_moments) {
  for (int64_t x = 0; x < n3; x++) out_moments[x] = 0.0;
  for (int64_t r = 0; r < n_reads; r++) {
    if (status[r] != 0) continue;
    for (int64_t x = 0; x < n3; x++) out_moments[x] = out_moments[x] + per_read[r * n3 + x];
  }
}
