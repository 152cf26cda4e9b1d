// The host arithmetic of the pipelined host-pointer path (pipeline.hip), in plain C++ so that it can be compiled
// and checked without a GPU (tests/host_shims/pipe_plan_host.cpp, tests/test_pipe_plan_cpu.py): which reads go
// into which chunk, where the arrays of a chunk lie inside its packed upload, and the offset arrays rebased to
// the chunk.  Nothing here touches HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pipe_plan {

enum { MAX_CHUNKS = 64 };  // (the clamp of NADAVCA_E2E_CHUNKS)

// Chunks.  What a single call can hide is bounded by its first upload (nothing to compute yet) and by how
// full the chip is while only the early chunks are in flight; so the chunks GROW: a small first one gets the
// kernels going early, each later one is `growth` times its predecessor's share of the signal bytes.  A chunk
// holds at least `floor_bytes` of signal and at least `min_reads` reads on average (the batch has fewer pieces
// otherwise), and a small batch stays in one piece.
// sig_off: n_reads + 1 offsets in samples (doubles).  bounds: room for 2 * MAX_CHUNKS values; chunk i is the reads
// [bounds[2 i], bounds[2 i + 1]).  -> the number of chunks (>= 1 for n_reads >= 1): they partition [0, n_reads)
// in order and none is empty.
inline int64_t chunk_schedule(const int64_t *sig_off, int64_t n_reads, int64_t n_chunks, double growth,
                              int64_t min_reads, int64_t floor_bytes, int64_t *bounds) {
  const int64_t total_sig = sig_off[n_reads];
  if (n_chunks > MAX_CHUNKS) n_chunks = MAX_CHUNKS;
  if (total_sig * 8 < n_chunks * floor_bytes) n_chunks = total_sig * 8 / floor_bytes;
  if (n_chunks > n_reads / min_reads) n_chunks = n_reads / min_reads;
  if (n_chunks < 1) n_chunks = 1;
  double wsum = 0.0, w = 1.0;
  for (int64_t c = 0; c < n_chunks; c++, w *= growth) wsum += w;
  int64_t lo = 0, made = 0;
  double wacc = 0.0;
  w = 1.0;
  for (int64_t c = 0; c < n_chunks; c++, w *= growth) {
    int64_t hi;
    wacc += w;
    if (c == n_chunks - 1) {
      hi = n_reads;
    } else {  // first read index whose signal offset reaches this chunk's cumulative share
      const int64_t target = (int64_t)((double)total_sig * (wacc / wsum));
      int64_t x = lo, y = n_reads;
      while (x < y) {
        const int64_t mid = (x + y) >> 1;
        if (sig_off[mid] < target) x = mid + 1; else y = mid;
      }
      hi = x > lo ? x : lo + 1;
      if (hi > n_reads) hi = n_reads;
    }
    if (hi <= lo) continue;
    bounds[2 * made] = lo;
    bounds[2 * made + 1] = hi;
    made++;
    lo = hi;
  }
  return made;
}

// The packed upload of a chunk of n reads: the five offset arrays (n + 1 int64 each: signal, reference,
// context_before, context_after, anchors), then the reference (tr int32), the contexts (tb, ta int32) and the
// anchors (tn pairs of int32).  at[q]: byte offset of array q; -> the size of the pack in bytes.
inline size_t pack_layout(int64_t n, int64_t tr, int64_t tb, int64_t ta, int64_t tn, size_t at[9]) {
  const size_t no = (size_t)(n + 1) * 8;
  const size_t sizes[9] = {no, no, no, no, no, (size_t)tr * 4, (size_t)tb * 4, (size_t)ta * 4, (size_t)tn * 8};
  size_t total = 0;
  for (int q = 0; q < 9; q++) {
    at[q] = total;
    total += (sizes[q] + 63) & ~(size_t)63;  // (a 64-byte granule keeps every array 16-byte aligned; empty arrays too)
    if (sizes[q] == 0) total += 64;
  }
  return total;
}

// The five offset arrays of reads [a, a + n) rebased to the chunk (each starts at 0), written into the pack image
// `buf` at at[0..4].
inline void rebase_offsets(const int64_t *const src[5], int64_t a, int64_t n, const size_t at[9], char *buf) {
  for (int q = 0; q < 5; q++) {
    int64_t *dst = (int64_t *)(buf + at[q]);
    const int64_t base = src[q][a];
    for (int64_t i = 0; i <= n; i++) dst[i] = src[q][a + i] - base;
  }
}

}  // namespace pipe_plan
