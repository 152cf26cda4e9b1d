// Host build of nadavca_amd/csrc/pipe_plan.h for tests/test_pipe_plan_cpu.py and tests/test_gpu_host_pipeline.py
// (g++ -O2 -ffp-contract=off -shared): the chunk schedule, pack layout and offset rebase that pipeline.hip runs.
#include "../../nadavca_amd/csrc/pipe_plan.h"

// bounds: room for 2 * 64 values -> number of chunks
extern "C" long long pipe_plan_host_schedule(const long long *sig_off, long long n_reads, long long n_chunks,
                                             double growth, long long min_reads, long long floor_bytes,
                                             long long *bounds) {
  static_assert(sizeof(long long) == sizeof(int64_t), "");
  return pipe_plan::chunk_schedule((const int64_t *)sig_off, n_reads, n_chunks, growth, min_reads, floor_bytes,
                                   (int64_t *)bounds);
}

// at: 9 values -> total bytes
extern "C" unsigned long long pipe_plan_host_layout(long long n, long long tr, long long tb, long long ta,
                                                    long long tn, unsigned long long *at) {
  size_t a[9];
  const size_t total = pipe_plan::pack_layout(n, tr, tb, ta, tn, a);
  for (int q = 0; q < 9; q++) at[q] = a[q];
  return total;
}

// the five offset arrays of reads [a, a + n) rebased into buf (laid out by at, as pipe_plan_host_layout gave it)
extern "C" void pipe_plan_host_rebase(const long long *sig_off, const long long *ref_off, const long long *cb_off,
                                      const long long *ca_off, const long long *anc_off, long long a, long long n,
                                      const unsigned long long *at, char *buf) {
  const int64_t *src[5] = {(const int64_t *)sig_off, (const int64_t *)ref_off, (const int64_t *)cb_off,
                           (const int64_t *)ca_off, (const int64_t *)anc_off};
  size_t a9[9];
  for (int q = 0; q < 9; q++) a9[q] = (size_t)at[q];
  pipe_plan::rebase_offsets(src, a, n, a9, buf);
}
