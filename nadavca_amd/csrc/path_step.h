// The path comparison of the forward sweep (kernels_align3.hip, "path step"): is the score a lane receives from the
// previous row strictly greater than the row's running maximum, at the resolution of the reference's log-doubles
// (xmath.h: gt_tol), and does the pair fall into one of the tie classes of the parity contract (include/nadavca_hip.h).
// Host-usable like ell_items.h (g++ build: tests/test_path_step_cpu.py).
//
// Inputs: the candidate (dv, Gin) and the running maximum (bestn, G), both (double, integer scale) pairs, stored =
// true * 2^scale; bestn is normalised to [0.5, 1), or 0 with G = GBIG while the row has no maximum yet.
//   dva    = dv * 2^(G - Gin)                  the candidate on the maximum's scale (0 stays 0, no maximum yet: +inf)
//   tdiff  = dva - bestn
//   margin = bestn * (|G| * 2^-52)             path_margin: one ulp of the reference's log value, as gt_tol has it
//   near   = |tdiff| < dva * 2^-24             the tie flag's margin (xmath.h: near_tol)
// Two forms of the same decision:
//   path_cmp_full   upd = tdiff > margin, and the tie class of a near pair — the arithmetic of gt_tol, every time
//   path_cmp_fast   near and upd = tdiff > 0 — no margin.  Where `near` is set the caller computes path_margin and takes
//                   upd = tdiff > margin and the class from path_tie_class (the kernel does so for the whole wave, in the
//                   block it enters when any lane is near); where it is not, upd is already right:
//
// LEMMA.  For |G| < 2^27 and a pair that is not near, tdiff > margin and tdiff > 0 are the same bit.
//   tdiff <= 0 or NaN: both are false (margin >= 0).
//   tdiff > 0, not near: tdiff >= dva * 2^-24 (the product is exact, a power of two) and dva > bestn, so
//     tdiff > bestn * 2^-24 >= bestn * |G| * 2^-52 * (1 + 2^-52) >= margin — (double)|G| * 2^-52 is exact, the product
//     with bestn rounds once.
//   No maximum yet (bestn = 0): margin = 0.  dva = +inf: tdiff = +inf, never near, greater than any margin.
//   dva * 2^-24 flushed to zero (this engine flushes FP64 denormals): never near; dva < 2^-998, so against a bestn in
//     [0.5, 1) tdiff < 0, and against bestn = 0 the margin is 0.
//   There is a bound: once |G| * 2^-52 > 2^-24 / (1 - 2^-24), a little above |G| = 2^28, there are pairs outside the
//   tie margin and inside gt_tol's (tests/test_path_step_cpu.py finds them at 2^29 and none at 2^28 itself).
// path_margin is a pure function of (bestn, G): computed where it is needed it is the double the sweep used to carry
// from the update on.
//
// The arg-max over the last row (path_top_margin) compares posteriors times scores that are not normalised: margin =
// fbest * (|exponent(fbest) - fG| * 2^-52); the same lemma holds with |exponent(fbest) - fG| in the place of |G|.
//
// THE BOUND.  A row's scale is the scale it received less the exponent of a normal double, and row 0 hands on scale 0,
// so one row moves |G| by at most 1024 and |G| <= 1024 * row whatever the data: a read of up to PATH_ROWS_PROVEN rows
// (2^17 less a few; the longest reads of any workload have ~10^4) stays below 2^27 everywhere, the last row's arg-max
// with its one exponent more included.  The sweep hands longer reads to the exact kernel, and, like any other range
// guard, a read in which a lane leaves a row with |G| >= PATH_G_GUARD = 2^26 — the row ends are where the best path's
// own exponent shows, long before the worst case of the induction is anywhere near.
#pragma once
#include <math.h>
#include <stdlib.h>
#ifdef __HIPCC__
#define PATH_STEP_FN __host__ __device__ inline
#else
#define PATH_STEP_FN inline
#endif
namespace path_step {
constexpr int GBIG = 1 << 24;          // scale of an empty running maximum: any dv > 0 becomes +inf on it
constexpr int PATH_G_GUARD = 1 << 26;  // a row left with |G| at or above this: the exact kernel redoes the read
constexpr int PATH_ROWS_PROVEN = (1 << 17) - 4;  // rows of a read: 1024 * (rows + 1) < 2^27
constexpr int TIE_BITS = 24;           // the tie flag's relative margin is 2^-24 (xmath.h: NVK_TIE_BITS)
constexpr int TIE_ULPS = 64;           // the ULP class: within this many margins (xmath.h: NVK_TIE_ULPS)
enum { TIE_NONE = 0, TIE_EXACT = 1, TIE_NEAR = 2, TIE_ULP = 4 };  // include/nadavca_hip.h: NVK_TIE_*

// v_frexp_mant_f64 / v_frexp_exp_i32_f64 / v_ldexp_f64 and their plain C++ forms.  The instructions return the
// operand and exponent 0 for 0, inf and NaN, and with FP64 denormals flushed (kernels_align3.hip is compiled so) a
// denormal operand or result is a zero: ftz() restates that on the host.
#ifdef __HIP_DEVICE_COMPILE__
PATH_STEP_FN double ftz(double x) { return x; }
PATH_STEP_FN double frexp_mant(double x) { return __builtin_amdgcn_frexp_mant(x); }
PATH_STEP_FN int frexp_exp(double x) { return __builtin_amdgcn_frexp_exp(x); }
PATH_STEP_FN double scale2(double x, int n) { return ldexp(x, n); }
#else
PATH_STEP_FN double ftz(double x) { return fabs(x) < 0x1.0p-1022 ? copysign(0.0, x) : x; }
PATH_STEP_FN double frexp_mant(double x) {
  int n;
  x = ftz(x);
  return (x == 0.0 || isinf(x) || isnan(x)) ? x : frexp(x, &n);
}
PATH_STEP_FN int frexp_exp(double x) {
  int n = 0;
  x = ftz(x);
  if (!(x == 0.0 || isinf(x) || isnan(x))) frexp(x, &n);
  return n;
}
PATH_STEP_FN double scale2(double x, int n) { return ftz(ldexp(ftz(x), n)); }
#endif

struct PathCmp {
  double dva, tdiff;
  bool near;  // inside the tie margin
  bool upd;   // the candidate replaces the maximum
  int cls;    // path_cmp_full: TIE_EXACT / TIE_ULP / TIE_NEAR of a near pair, else TIE_NONE
};

PATH_STEP_FN double path_margin(double bestn, int G) { return ftz(bestn * ((double)abs(G) * 0x1.0p-52)); }
// (the last row's arg-max: fbest is a posterior times a score, fG its scale)
PATH_STEP_FN double path_top_margin(double fbest, int fG) {
  return ftz(fbest * ((double)abs(frexp_exp(fbest) - fG) * 0x1.0p-52));
}
PATH_STEP_FN bool path_near(double tdiff, double dva) {
  return fabs(tdiff) < ftz(dva * (1.0 / (double)(1ull << TIE_BITS)));
}
PATH_STEP_FN bool path_tie_exact(double tdiff) { return tdiff == 0.0; }
PATH_STEP_FN bool path_tie_ulp(double tdiff, double margin) { return fabs(tdiff) <= ftz(margin * (double)TIE_ULPS); }
// the class of a near pair
PATH_STEP_FN int path_tie_class(double tdiff, double margin) {
  return path_tie_exact(tdiff) ? TIE_EXACT : path_tie_ulp(tdiff, margin) ? TIE_ULP : TIE_NEAR;
}

PATH_STEP_FN PathCmp path_cmp_fast(double dv, int Gin, double bestn, int G) {
  PathCmp c;
  c.dva = scale2(dv, G - Gin);
  c.tdiff = ftz(c.dva - bestn);
  c.near = path_near(c.tdiff, c.dva);
  c.upd = c.tdiff > 0.0;  // (dv == 0 outside the span: never an update)
  c.cls = TIE_NONE;
  return c;
}
// what the caller of path_cmp_fast does for a pair that is near (the sweep: for every lane, once any lane is)
PATH_STEP_FN void path_cmp_cold(PathCmp &c, double bestn, int G) {
  const double margin = path_margin(bestn, G);
  c.upd = c.tdiff > margin;
  c.cls = c.near ? path_tie_class(c.tdiff, margin) : TIE_NONE;
}
PATH_STEP_FN PathCmp path_cmp_full(double dv, int Gin, double bestn, int G) {
  PathCmp c = path_cmp_fast(dv, Gin, bestn, G);
  path_cmp_cold(c, bestn, G);
  return c;
}
// the maximum after an update by dv: mantissa in [0.5, 1) and its scale; -G = true exponent
PATH_STEP_FN void path_take(double dv, int Gin, double &bestn, int &G) {
  bestn = frexp_mant(dv);
  G = Gin - frexp_exp(dv);
}
}  // namespace path_step
