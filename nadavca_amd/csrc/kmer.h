// The k-mer id of a position of a read: the one restatement of the reference's extended-sequence lookup
// (nadavca/dtw/sequence.cpp:6-38) and of KmerModel's index (kmer_model.cpp:22-30) that every kernel uses.
// Of `dm` only the window's shape is read: k, central, alphabet.
#pragma once
#include "nvk_internal.h"

// ExtendedSequence::operator[] : context_before | reference | context_after, 0 outside
__device__ __forceinline__ int seq_at(const int32_t *ref, int R, const int32_t *cb, int nb,
                                      const int32_t *ca, int na, int idx) {
  if (idx < 0) {
    int j = idx + nb;
    return j >= 0 ? cb[j] : 0;
  }
  if (idx < R) return ref[idx];
  int j = idx - R;
  return j < na ? ca[j] : 0;
}

// k-mer id of position pos; where sub(j, v) is true, v replaces the base at position j of the window (a hypothesis'
// substitutions, sequence.cpp:31-38)
template <class Sub>
__device__ __forceinline__ int64_t kmer_id(const DeviceModel &dm, const int32_t *ref, int R,
                                           const int32_t *cb, int nb, const int32_t *ca, int na,
                                           int pos, const Sub &sub) {
  int64_t id = 0;
  for (int j = pos - dm.central; j < pos - dm.central + dm.k; j++) {
    int v;
    if (!sub(j, v)) v = seq_at(ref, R, cb, nb, ca, na, j);
    id = id * dm.alphabet + v;
  }
  return id;
}
__device__ __forceinline__ int64_t kmer_id(const DeviceModel &dm, const int32_t *ref, int R,
                                           const int32_t *cb, int nb, const int32_t *ca, int na,
                                           int pos) {
  return kmer_id(dm, ref, R, cb, nb, ca, na, pos, [](int, int &) { return false; });
}

// k-mer id of position pos of an EDITED sequence (an insertion / deletion hypothesis): map(j, v) either gives the
// letter v at position j of the edited sequence and returns true (an inserted base), or rewrites j to the position of
// the unedited sequence that base comes from (contexts included: before 0, from R on) and returns false
template <class Map>
__device__ __forceinline__ int64_t kmer_id_mapped(const DeviceModel &dm, const int32_t *ref, int R,
                                                  const int32_t *cb, int nb, const int32_t *ca, int na,
                                                  int pos, const Map &map) {
  int64_t id = 0;
  for (int j = pos - dm.central; j < pos - dm.central + dm.k; j++) {
    int v, src = j;
    if (!map(src, v)) v = seq_at(ref, R, cb, nb, ca, na, src);
    id = id * dm.alphabet + v;
  }
  return id;
}

// kmer_id, or -1 when a base code anywhere in the window is outside 0 .. alphabet-1: no table entry exists (the
// reference indexes out of bounds there)
__device__ __forceinline__ int64_t kmer_id_checked(const DeviceModel &dm, const int32_t *ref, int R,
                                                   const int32_t *cb, int nb, const int32_t *ca, int na,
                                                   int pos) {
  int64_t id = 0;
  for (int j = pos - dm.central; j < pos - dm.central + dm.k; j++) {
    const int b = seq_at(ref, R, cb, nb, ca, na, j);
    if ((unsigned)b >= (unsigned)dm.alphabet) return -1;
    id = id * dm.alphabet + b;
  }
  return id;
}

// alphabet^k, the entries of a k-mer table, or -1 when k / alphabet are outside the served range
constexpr int MAX_K = 16;  // longest k-mer whose key fits the check below (alphabet^k <= 2^31)
inline int64_t kmer_table_size(int k, int alphabet) {
  if (k < 1 || k > MAX_K || alphabet < 1 || alphabet > 64) return -1;
  int64_t n = 1;
  for (int i = 0; i < k; i++) {
    n *= alphabet;
    if (n > ((int64_t)1 << 31)) return -1;
  }
  return n;
}
