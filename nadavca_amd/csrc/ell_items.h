// The packed hypotheses ("items") of the joint and the edit variant of ell_kernel (kernels_ell.hip): every shift and
// mask of the two codes, the checks of a list entry, the rows it re-runs and the index map of an edit (g++ build:
// tests/test_ell_items_cpu.py).  At most JOINT_ROWS rows first .. last are re-run (a 16-lane group less role 0 and the
// closing lane); back / fwd = k - central - 1 / central.  A letter takes 3 bits (alphabet <= 8: launch_ell).
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#define ELL_ITEMS_FN __host__ __device__ inline
#else
#define ELL_ITEMS_FN inline
#endif
namespace ell_items {
constexpr int JOINT_ROWS = 14, EDIT_MAX_INS = 13, EDIT_MAX_DEL = 255;
typedef unsigned long long code_t;
ELL_ITEMS_FN int lower(int a, int b) { return a < b ? a : b; }
ELL_ITEMS_FN int upper(int a, int b) { return a > b ? a : b; }
ELL_ITEMS_FN int code_lo(code_t code) { return (int)(unsigned)code; }
ELL_ITEMS_FN int code_hi(code_t code) { return (int)(unsigned)(code >> 32); }
ELL_ITEMS_FN code_t code_of(int lo, int hi) { return ((code_t)(unsigned)hi << 32) | (unsigned)lo; }
// ---- joint items: the effective substitutions (b != ref[p]) of a hypothesis as its first position p1 and one nibble
// per offset from p1 (bit 3: substituted, bits 0-2: the letter); the offsets stay below JOINT_ROWS, so nibble 15 is
// free and holds the last offset.  A hypothesis without an effective substitution is code 0.
ELL_ITEMS_FN int joint_span(code_t code) { return (int)(code >> 60); }  // last substituted position - p1
ELL_ITEMS_FN int joint_first(int p1, int back) { return upper(0, p1 - back); }
ELL_ITEMS_FN int joint_last(int R, int plast, int fwd) { return lower(R - 1, plast + fwd); }
ELL_ITEMS_FN int joint_rows(int R, int back, int fwd, int p1, code_t code) {
  return code == 0 ? 0 : joint_last(R, p1 + joint_span(code), fwd) - joint_first(p1, back) + 1;
}
// the letter v that replaces the base at position j, or false
ELL_ITEMS_FN bool joint_at(int p1, code_t code, int j, int &v) {
  const unsigned o = (unsigned)(j - p1);
  const int nib = o < (unsigned)JOINT_ROWS ? (int)(code >> (4 * o)) & 15 : 0;
  v = nib & 7;
  return (nib & 8) != 0;
}
// Packs the n substitutions (pos[s], base[s]) of a hypothesis of the read `ref`, dropping those that change nothing.
// false: refused — positions not strictly ascending or outside the read, a letter outside the alphabet, too many rows
ELL_ITEMS_FN bool joint_pack(const int32_t *ref, int R, int alphabet, int back, int fwd, const int32_t *pos,
                             const int32_t *base, int64_t n, int &p1, code_t &code, int &rows) {
  int prev = -1, plast = 0;
  bool ok = true;
  p1 = 0;
  code = 0;
  for (int64_t s = 0; s < n; s++) {
    const int sp = pos[s], sb = base[s];
    ok = sp > prev && sp < R && sb >= 0 && sb < alphabet;  // (prev >= -1: also sp >= 0)
    if (!ok) break;
    prev = sp;
    if (sb == ref[sp]) continue;
    if (code == 0) p1 = sp;
    ok = sp - p1 < JOINT_ROWS;  // or more rows than a group has lanes for, wherever the read ends
    if (!ok) break;
    code |= (code_t)(8 | sb) << (4 * (sp - p1));
    plast = sp;
  }
  if (code != 0) code |= (code_t)(plast - p1) << 60;
  rows = joint_rows(R, back, fwd, p1, code);
  return ok && rows <= JOINT_ROWS;
}
// ---- edit items: the hypothesis (p, d, s), i = len(s): delete d bases from p on, put the letters s in their place.
// The code holds one nibble per letter (at most EDIT_MAX_INS: i letters re-run at least i + 1 rows), i in bits 52-55
// and d in bits 56-63.  (d, i) = (0, 0) is code 0.  The edited reference ref' = ref[:p] + s + ref[p+d:] has R - d + i
// bases; a base of the read stays on either side of the edit: 1 <= p and p + d <= R - 1.
struct Edit { int p, i, d; code_t code; };
ELL_ITEMS_FN Edit edit_unpack(int p, code_t code) { return Edit{p, (int)(code >> 52) & 15, (int)(code >> 56), code}; }
// back = 0: row p - 1 too, the band of its emitting row (boundary row p) changes
ELL_ITEMS_FN int edit_first(const Edit &e, int back) { return upper(0, lower(e.p - 1, e.p - back)); }
ELL_ITEMS_FN int edit_last(const Edit &e, int R, int fwd) { return lower(R - e.d + e.i - 1, e.p + e.i - 1 + fwd); }
ELL_ITEMS_FN int edit_rows(const Edit &e, int R, int back, int fwd) { return edit_last(e, R, fwd) - edit_first(e, back) + 1; }
// The edit map.  Position / boundary row r of ref' behind the edit (r >= p + i) is the read's r - i + d ...
ELL_ITEMS_FN int edit_behind(const Edit &e, int r) { return r - e.i + e.d; }
// ... so position j of ref' is the letter v (true), or the base of the read (contexts included) that j is rewritten to
ELL_ITEMS_FN bool edit_at(const Edit &e, int &j, int &v) {
  const unsigned o = (unsigned)(j - e.p);
  v = (int)(e.code >> (4 * (o & 15))) & 7;
  if (j >= e.p) j = edit_behind(e, j);
  return o < (unsigned)e.i;
}
// Boundary row r of ref' as a row of the read's bands: an inserted row starts as row p - 1 and ends as row p + d do
ELL_ITEMS_FN int edit_row_s(const Edit &e, int r) { return r < e.p ? r : r < e.p + e.i ? e.p - 1 : edit_behind(e, r); }
ELL_ITEMS_FN int edit_row_e(const Edit &e, int r) { return r < e.p ? r : r < e.p + e.i ? e.p + e.d : edit_behind(e, r); }
// boundary row last + 1 lies behind the edit: the read's row whose band and suffix row close the hypothesis
ELL_ITEMS_FN int edit_close(const Edit &e, int last) { return edit_behind(e, last + 1); }
// Packs the edit (p, d, s[0 .. ni)), ni >= 0.  false: refused — outside the read or the code's fields, a bad letter, rows
ELL_ITEMS_FN bool edit_pack(int R, int alphabet, int back, int fwd, int p, int d, const int32_t *s, int64_t ni,
                            code_t &code, int &rows) {
  code = 0, rows = 0;
  if (p < 1 || d < 0 || d > EDIT_MAX_DEL || ni > EDIT_MAX_INS || p > R - 1 - d) return false;
  for (int t = 0; t < (int)ni; t++) {
    if (s[t] < 0 || s[t] >= alphabet) return false;
    code |= (code_t)(s[t] & 7) << (4 * t);
  }
  code |= (code_t)ni << 52 | (code_t)d << 56;
  rows = edit_rows(edit_unpack(p, code), R, back, fwd);
  return rows <= JOINT_ROWS;
}
}  // namespace ell_items
