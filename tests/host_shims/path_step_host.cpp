// Host build of nadavca_amd/csrc/path_step.h for tests/test_path_step_cpu.py (g++, a ctypes library; also included by
// path_step_main.cpp, the stand-alone program the same cases go through under the sanitizers).
//
// path_step_host_run(n, dv, Gin, bestn, G, out): case j is the candidate (dv[j], Gin[j]) against the maximum
// (bestn[j], G[j]); out[j] packs what the two forms of the comparison find:
//   bit 0      path_cmp_full: upd             bits 1-3   path_cmp_full: class (TIE_EXACT | TIE_NEAR | TIE_ULP)
//   bit 4      fast + cold-block rule: upd    bits 5-7   fast + cold-block rule: class
//   bit 8      path_cmp_fast: near            bit 9      path_cmp_fast: upd (tdiff > 0, before the cold block)
// The cold-block rule is the sweep's: a pair that is near takes the margin, one that is not keeps tdiff > 0.
// Returns the number of cases whose two halves differ.
//
// path_step_host_take(dv, Gin, out_bestn, out_G): the maximum after an update (path_take).
#include <stdint.h>

#include "../../nadavca_amd/csrc/path_step.h"

extern "C" long long path_step_host_run(long long n, const double *dv, const int32_t *Gin, const double *bestn,
                                        const int32_t *G, int32_t *out) {
  long long differ = 0;
  for (long long j = 0; j < n; j++) {
    const path_step::PathCmp full = path_step::path_cmp_full(dv[j], Gin[j], bestn[j], G[j]);
    path_step::PathCmp fast = path_step::path_cmp_fast(dv[j], Gin[j], bestn[j], G[j]);
    const int near = fast.near ? 1 : 0, upd0 = fast.upd ? 1 : 0;
    if (fast.near) path_step::path_cmp_cold(fast, bestn[j], G[j]);
    const int a = (full.upd ? 1 : 0) | (full.cls << 1), b = (fast.upd ? 1 : 0) | (fast.cls << 1);
    out[j] = a | (b << 4) | (near << 8) | (upd0 << 9);
    differ += (a != b);
  }
  return differ;
}

extern "C" void path_step_host_take(double dv, int Gin, double *out_bestn, int32_t *out_G) {
  double bestn = 0.0;
  int G = path_step::GBIG;
  path_step::path_take(dv, Gin, bestn, G);
  *out_bestn = bestn;
  *out_G = G;
}

extern "C" double path_step_host_margin(double bestn, int G) { return path_step::path_margin(bestn, G); }
extern "C" double path_step_host_top_margin(double fbest, int fG) { return path_step::path_top_margin(fbest, fG); }
