// Host build of nadavca_amd/csrc/ell_items.h for tests/test_ell_items_cpu.py (g++, a ctypes library; also included by
// ell_items_main.cpp, the stand-alone program the same cases go through under the sanitizers).  One call evaluates one
// case through every function of the header and writes what it found as a flat list of integers:
//   refused: [0]
//   edit:    [1, code, i, d, rows, first, last, close, code_of(code_lo, code_hi) == code,
//             row_s[0 .. R'], row_e[0 .. R'],  (letter, 0) or (-1, source position) for at in [-PAD, R' + PAD)]
//   joint:   [1, code, p1, span, rows, first, last, code_of(code_lo, code_hi) == code,
//             letter or -1 for j in [-PAD, R + PAD)]          (first = last = 0 for code 0)
#include <stdint.h>

#include "../../nadavca_amd/csrc/ell_items.h"

enum { ELL_ITEMS_PAD = 9 };

extern "C" long long ell_items_host_edit(int R, int alphabet, int back, int fwd, int p, int d, const int32_t *s,
                                         long long ni, long long *out) {
  ell_items::code_t code;
  int rows;
  long long n = 0;
  if (!ell_items::edit_pack(R, alphabet, back, fwd, p, d, s, ni, code, rows)) {
    out[n++] = 0;
    return n;
  }
  const ell_items::Edit e = ell_items::edit_unpack(p, code);
  const int last = ell_items::edit_last(e, R, fwd), R2 = R - e.d + e.i;
  out[n++] = 1;
  out[n++] = (long long)code;
  out[n++] = e.i;
  out[n++] = e.d;
  out[n++] = ell_items::edit_rows(e, R, back, fwd) == rows ? rows : -1;
  out[n++] = ell_items::edit_first(e, back);
  out[n++] = last;
  out[n++] = ell_items::edit_close(e, last);
  out[n++] = ell_items::code_of(ell_items::code_lo(code), ell_items::code_hi(code)) == code;
  for (int r = 0; r <= R2; r++) out[n++] = ell_items::edit_row_s(e, r);
  for (int r = 0; r <= R2; r++) out[n++] = ell_items::edit_row_e(e, r);
  for (int at = -ELL_ITEMS_PAD; at < R2 + ELL_ITEMS_PAD; at++) {
    int j = at, v = -1;
    const bool letter = ell_items::edit_at(e, j, v);
    out[n++] = letter ? v : -1;
    out[n++] = letter ? 0 : j;
  }
  return n;
}

extern "C" long long ell_items_host_joint(const int32_t *ref, int R, int alphabet, int back, int fwd,
                                          const int32_t *pos, const int32_t *base, long long ns, long long *out) {
  ell_items::code_t code;
  int p1, rows;
  long long n = 0;
  if (!ell_items::joint_pack(ref, R, alphabet, back, fwd, pos, base, ns, p1, code, rows)) {
    out[n++] = 0;
    return n;
  }
  const int span = ell_items::joint_span(code);
  out[n++] = 1;
  out[n++] = (long long)code;
  out[n++] = p1;
  out[n++] = span;
  out[n++] = ell_items::joint_rows(R, back, fwd, p1, code) == rows ? rows : -1;
  out[n++] = code ? ell_items::joint_first(p1, back) : 0;
  out[n++] = code ? ell_items::joint_last(R, p1 + span, fwd) : 0;
  out[n++] = ell_items::code_of(ell_items::code_lo(code), ell_items::code_hi(code)) == code;
  for (int j = -ELL_ITEMS_PAD; j < R + ELL_ITEMS_PAD; j++) {
    int v = -1;
    out[n++] = ell_items::joint_at(p1, code, j, v) ? v : -1;
  }
  return n;
}
