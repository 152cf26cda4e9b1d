// numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, @TYPE@_pairwise_sum), restated for one GPU
// thread: np_sum equals numpy.add.reduce of a contiguous float64 vector bit for bit (tests/test_renorm_cpu.py checks
// this order against numpy itself).  Used by the event means and the linear fit (kernels_renorm.hip) and by the k-mer
// statistics (kernels_kmerstats.hip) and the site levels (kernels_sitelevels.hip).
//
// The sums run over a generated sequence f(0 .. n), not over an array: the squared deviations and the gathered values
// of the k-mer statistics are never stored.  The walk's stack is in registers: every access to it is an unrolled
// select over its 8 frames, so it needs no scratch memory (a walk with indexed stack arrays cost event_means_kernel
// 112 B of scratch per lane and linfit_kernel 166 VGPRs).
// Resource use (gfx950, -Rpass-analysis=kernel-resource-usage): kmer_event_kernel 72 / 74 VGPRs and 78 / 80 SGPRs
// (pass 1 / pass 2), its long_event_kernel 82 / 84 VGPRs and 99 / 103 SGPRs, kmer_reduce_kernel 86 VGPRs and 99 SGPRs;
// no LDS, no scratch, no spills.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <class F>
__device__ __forceinline__ double np_block_sum(const F &f, int o, int n) {  // n <= 128
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; i++) res += f(o + i);
    return res;
  }
  double r0 = f(o + 0), r1 = f(o + 1), r2 = f(o + 2), r3 = f(o + 3);
  double r4 = f(o + 4), r5 = f(o + 5), r6 = f(o + 6), r7 = f(o + 7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += f(o + i + 0); r1 += f(o + i + 1); r2 += f(o + i + 2); r3 += f(o + i + 3);
    r4 += f(o + i + 4); r5 += f(o + i + 5); r6 += f(o + i + 6); r7 += f(o + i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; i++) res += f(o + i);
  return res;
}

__device__ __forceinline__ int np_split(int m) {  // left half of a node of m > 128 elements
  int n2 = m / 2;
  return n2 - n2 % 8;
}

// sum(a, n) = sum(a, n2) + sum(a + n2, n - n2) down to blocks of <= 128, n <= 8192: a node of m elements has
// children of at most m/2 + 8, so a path from the root holds at most 7 internal nodes.  The walk keeps the path as
// bits (bit i: the node at depth i + 1 is a right child), rebuilds a node's offset and size from them when it needs
// them, and keeps the left sums of the path's nodes in sv.
template <class F>
__device__ double np_pairwise_sum(const F &f, int o0, int n) {
  if (n <= 128) return np_block_sum(f, o0, n);
  constexpr int D = 8;
  double sv[D];
#pragma unroll
  for (int i = 0; i < D; i++) sv[i] = 0.0;
  unsigned path = 0;
  int d = 0, o = o0, m = n;  // the current node and its depth
  for (;;) {
    while (m > 128) {  // descend left
      m = np_split(m);
      path &= ~(1u << d);
      d++;
    }
    double ret = np_block_sum(f, o, m);
    for (;;) {  // ascend until a node still has its right child to do
      if (d == 0) return ret;
      d--;
      if (!((path >> d) & 1u)) {  // the left child of the node at depth d is done: keep it, go right
#pragma unroll
        for (int i = 0; i < D; i++)
          if (i == d) sv[i] = ret;
        int po = o0, pm = n;
        for (int i = 0; i < d; i++) {
          const int n2 = np_split(pm);
          if ((path >> i) & 1u) { po += n2; pm -= n2; } else { pm = n2; }
        }
        const int n2 = np_split(pm);
        path |= 1u << d;
        d++;
        o = po + n2;
        m = pm - n2;
        break;
      }
      double pv = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++)
        if (i == d) pv = sv[i];
      ret = pv + ret;
    }
  }
}

// numpy.add.reduce of a contiguous float64 vector: the reduction loop receives the data in pieces of 8192 elements
// (numpy's buffer size), each summed pairwise and added to the running result, which starts at 0
template <class F>
__device__ double np_sum(const F &f, int64_t n) {
  double res = 0.0;
  for (int64_t o = 0; o < n; o += 8192) {
    const int64_t base = o;
    auto g = [&](int i) { return f(base + i); };
    res = res + np_pairwise_sum(g, 0, (int)(n - o < 8192 ? n - o : 8192));
  }
  return res;
}
__device__ __forceinline__ double np_sum(const double *a, int64_t n) {
  return np_sum([a](int64_t i) { return a[i]; }, n);
}
